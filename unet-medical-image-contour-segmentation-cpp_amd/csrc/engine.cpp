// engine.cpp -- the C-ABI of include/mi_unet.h: the handle (create / clone / destroy), weight adoption, the numeric guard, the
// launches of the forward plan and their graph replay, the u8, postprocess and contour entry points.  The RAW-in and tiled entry
// points are pipeline_raw.cpp and pipeline_tiled.cpp, the debug entry points debug.cpp; weights.cpp packs, plan.cpp plans.
// Host code only; every device kernel lives in the .hip files next to it.
//
// Replaces, for the reference's hot path, initialize_engine's engine deserialisation (src/initialize.cpp:49-60),
// initialize_context's buffers/stream (src/process.cpp:45-120) and execute_inference (src/process.cpp:123-175).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>

#include "engine_handle.h"

using namespace miunet;

namespace miunet {

PlanInput plan_input(const mi_unet *h)
{
    PlanInput in;
    in.cfg = h->cfg; in.algo = h->algo; in.fuse_pool = h->fuse_pool; in.fuse_head = h->fuse_head;
    in.weights = h->d_weights;
    for (int i = 0; i < 8; ++i) { in.cat[i] = h->d_cat[i]; in.cat_floats[i] = h->cat_floats[i]; }
    in.s0 = h->d_s0; in.s1 = h->d_s1; in.s_floats = h->s_floats;
    in.routing = h->routing; in.guard_tripped = h->wino4_guard_tripped; in.wino4_min_wg = h->wino4_min_wg;
    in.lut = h->d_lut; in.ksplit = h->d_ksplit; in.ksplit_bytes = h->ksplit_bytes;
    return in;
}

// An executable leaves the graph cache (eviction, new weights, destroy).  The device entry point returns once it has enqueued, so a
// replay of `exec` may still be in flight on the stream of its key; destroying it then is not something the runtime promises to
// defer.  That stream is the handle's current one or its own, which are alive and are waited for directly, or a caller's stream the
// handle was switched away from: the caller may have destroyed that one since, so the wait is for the event that mi_unet_set_stream
// recorded on it at the switch, behind everything this handle enqueued there.  Not on the path of a cached key.
void GraphRetire::operator()(const GraphKey &key, hipGraphExec_t exec) const
{
    if (key.stream == h->stream || key.stream == h->own_stream) {
        (void)hipStreamSynchronize(static_cast<hipStream_t>(const_cast<void *>(key.stream)));
    } else {
        for (const mi_unet::LeftStream &l : h->left_streams)
            if (l.stream == key.stream) (void)hipEventSynchronize(l.done);
    }
    (void)hipGraphExecDestroy(exec);
}

int run_microbatch(mi_unet *h, const uint8_t *d_imgs, int B, uint8_t *d_labels, float *d_logits)
{
    if (!h->use_graph || h->profiling) return launch_plan(h, d_imgs, B, d_labels, d_logits);
    hipStream_t s = h->stream;
    const GraphKey key{ s, d_imgs, d_labels, d_logits, B };
    mi_unet::GraphCache::Entry *ge = h->graphs.find(key);
    if (!ge) ge = &h->graphs.insert(key);                // at 64 entries in the oldest one's place: GraphRetire below
    if (ge->exec) {
        HIP_TRY(hipGraphLaunch(ge->exec, s));
        return 0;
    }
    if (ge->uses++ == 0) return launch_plan(h, d_imgs, B, d_labels, d_logits);   // eager once (also sets kernel attributes)
    hipGraph_t graph = nullptr;
    HIP_TRY(hipStreamBeginCapture(s, hipStreamCaptureModeThreadLocal));
    const int rc = launch_plan(h, d_imgs, B, d_labels, d_logits);
    const hipError_t e = hipStreamEndCapture(s, &graph);
    if (rc) { if (graph) (void)hipGraphDestroy(graph); return rc; }
    if (e != hipSuccess) return fail(MI_UNET_EHIP, std::string("hipStreamEndCapture: ") + hipGetErrorString(e));
    const hipError_t ei = hipGraphInstantiate(&ge->exec, graph, nullptr, nullptr, 0);
    (void)hipGraphDestroy(graph);
    if (ei != hipSuccess) { ge->exec = nullptr; return fail(MI_UNET_EHIP, std::string("hipGraphInstantiate: ") + hipGetErrorString(ei)); }
    HIP_TRY(hipGraphLaunch(ge->exec, s));
    return 0;
}

hipError_t launch_route(Route r, const ConvArgs &a, const AsmKernels *k, hipStream_t s)
{
    switch (r) {
#define MIUNET_ROUTE_LAUNCH(id, name, call) case Route::id: return call;
        MIUNET_ROUTES(MIUNET_ROUTE_LAUNCH)
#undef MIUNET_ROUTE_LAUNCH
    }
    return hipErrorInvalidValue;
}

int grow_events(std::vector<Event> &ev, size_t n)
{
    while (ev.size() < n) {
        ev.emplace_back();
        HIP_TRY(ev.back().reset());
    }
    return 0;
}

int launch_plan(mi_unet *h, const uint8_t *d_imgs, int B, uint8_t *d_labels, float *d_logits)
{
    hipStream_t s = h->stream;
    const int lp_kind = h->algo == MI_UNET_CONV_BF16 ? 1 : h->algo == MI_UNET_CONV_FP16 ? 2 : 0;
    std::vector<Launch> launches;
    route_plan(plan_input(h), h->plan, d_imgs, B, d_labels, d_logits, lp_kind, launches);
    for (size_t i = 0; i < h->plan.size(); ++i) {
        const Step &st = h->plan[i];
        const Launch &l = launches[i];
        const bool tapped = h->tap.layer == (int)i;
        if (l.skip) {
            if (tapped) { h->tap.info->skipped = 1; h->tap.hit = true; return 0; }
            continue;
        }
        if (tapped)
            if (int rc = tap_input(h, st, l, d_imgs, lp_kind)) return rc;
        hipEvent_t e0 = nullptr, e1 = nullptr;
        if (h->profiling) {
            if (int rc = grow_events(h->ev_pool, h->ev_used + 2)) return rc;
            e0 = h->ev_pool[h->ev_used++];
            e1 = h->ev_pool[h->ev_used++];
            HIP_TRY(hipEventRecord(e0, s));
        }
        hipError_t e;
        switch (l.rc.route) {
        case Route::FIRST:
            e = launch_conv3x3_first(d_imgs, h->d_lut, st.w, st.shift, st.dst, B, st.H, st.W, st.C, st.Cout, st.ld, lp_kind, h->routing, s);
            break;
        case Route::POOL:
            e = lp_kind ? launch_maxpool2x2_u16(st.src, st.ld, st.dst, B, st.H, st.W, st.C, s)
                        : launch_maxpool2x2(st.src, st.ld, st.dst, B, st.H, st.W, st.C, s);
            break;
        case Route::HEAD:
            e = launch_head_argmax(st.src, st.C, st.w, st.shift, st.Cout, d_logits, d_labels, B, st.H * st.W, s);
            break;
        case Route::UPSAMPLE:
            e = launch_upsample2x_bilinear(st.src, st.C, st.dst, st.ld, st.co_off, B, st.H, st.W, st.C, lp_kind, h->routing, s);
            break;
        default:
            e = launch_route(l.rc.route, l.a, h->asm_kernels.get(), s);
        }
        if (e != hipSuccess) return fail(MI_UNET_EHIP, "launch " + st.name + ": " + hipGetErrorString(e));
        if (tapped) {
            if (int rc = tap_output(h, st, l, d_labels, d_logits, lp_kind)) return rc;
            h->tap.hit = true;
            return 0;
        }
        if (h->profiling) {
            HIP_TRY(hipEventRecord(e1, s));
            mi_unet_kernel_stat ks{};
            snprintf(ks.name, sizeof ks.name, "%s", st.name.c_str());
            snprintf(ks.kernel, sizeof ks.kernel, "%s", route_name(l.rc.route, l.rc.fused).c_str());
            ks.flops = st.flops_per_img * B;
            // algorithmic bytes: the 16-bit pipelines move half of them (activations and weights are 2 bytes)
            ks.bytes = (st.bytes_per_img * B + st.weight_bytes) *
                       ((lp_kind && (st.kind == Step::CONV || st.kind == Step::CONVT || st.kind == Step::UPSAMPLE)) ? 0.5 : 1.0);
            if (l.rc.fused & FUSE_FIRST) {        // + the first layer's arithmetic; the image in place of its output tensor
                const Step &f = h->plan[0];
                ks.flops += f.flops_per_img * B;
                ks.bytes += ((double)f.H * f.W * f.C - (lp_kind ? 2.0 : 4.0) * st.a.H * st.a.W * st.a.Cin) * B;
            }
            ks.ms = -1.f;                      // filled by mi_unet_get_kernel_stats
            h->stats.push_back(ks);
        }
    }
    return 0;
}

// postprocess_mask on the device, in place on `d_labels`; the network's scratch buffer s1 is free once the head has run
static int device_postprocess(mi_unet *h, uint8_t *d_labels, int B)
{
    const int H = h->cfg.height, W = h->cfg.width;
    const size_t cap = sizeof(float) * (size_t)h->cfg.max_batch * H * W * h->ch[0];
    if (postprocess_workspace_bytes(B, H, W) > cap) return fail(MI_UNET_EARG, "postprocess workspace does not fit the scratch buffer");
    return enqueue_tail(h, d_labels, B, H, W, default_targets(H, W), d_labels, h->d_s1, nullptr, nullptr, h->stream);
}

int enqueue_tail(mi_unet *h, const uint8_t *d_labels, int B, int H, int W, const TargetTable &t, uint8_t *d_planes, void *ws,
                 const ContourLayout *cl, hipEvent_t between, hipStream_t s, const std::string &where, const MeasureArgs *m)
{
    hipError_t e = t.K > 0 ? launch_postprocess_masks_multi(d_labels, d_planes, B, H, W, t, ws, s) : hipSuccess;
    if (e != hipSuccess) return fail(MI_UNET_EHIP, where + "postprocess launch: " + hipGetErrorString(e));
    if (between) HIP_TRY(hipEventRecord(between, s));
    if (!cl) return 0;
    int *const d_cont = h->d_cont;
    e = launch_mask_to_image_binary(d_planes, d_planes, (size_t)cl->planes * H * W, s);
    if (e == hipSuccess)
        e = launch_extract_contours(d_planes, cl->planes, H, W, cl->xy(d_cont), cl->cap_points, cl->start(d_cont), cl->cap_contours,
                                    cl->count(d_cont), ws, s);
    if (e != hipSuccess) return fail(MI_UNET_EHIP, where + "segment launch: " + hipGetErrorString(e));
    if (m) {                                             // the measuring half, on the forest and the sorted roots the contours came from
        const RegionLayout rl{ cl->planes, cl->cap_contours };
        uint8_t *const d_reg = h->d_regions;
        e = launch_measure_regions(cl->planes, H, W, t.K, m->d_tiles, h->cfg.in_ch, h->measure.channel, rl.regions(d_reg), rl.counts(d_reg),
                                   cl->cap_contours, ws, s);
        if (e != hipSuccess) return fail(MI_UNET_EHIP, where + "region launch: " + hipGetErrorString(e));
        HIP_TRY(hipMemcpyAsync(h->h_regions[m->half], d_reg, rl.bytes(), hipMemcpyDeviceToHost, s));
    }
    return 0;
}

TargetTable target_table(const mi_unet_target *targets, int n, int H, int W)
{
    TargetTable t;
    t.K = n;
    for (int k = 0; k < n; ++k) {
        t.cls[k] = targets[k].cls;
        t.min_area[k] = mi_unet_target_min_area(H, W, targets[k].min_area_frac);       // src/postprocess.cpp:9, :30, :66 (evaluated in float)
    }
    return t;
}

void table_morph(TargetTable &t, const mi_unet_morph *m, int n)
{
    for (int k = 0; k < t.K; ++k) {
        const mi_unet_morph &e = m[n == 1 ? 0 : k];
        t.shape[k] = e.shape; t.open_r[k] = e.open_r; t.close_r[k] = e.close_r;
    }
}

int check_morph_list(const mi_unet *h, const char *fn)
{
    if (h->n_morph == 1 || h->n_morph == h->n_targets) return 0;
    return fail(MI_UNET_ESTATE, std::string(fn) + ": the morphology list has " + std::to_string(h->n_morph) + " entries, the target list " +
                                    std::to_string(h->n_targets) + " (mi_unet_set_morph takes 1 entry or one per target)");
}

TargetTable target_table(const mi_unet *h, int H, int W)
{
    TargetTable t = target_table(h->targets, h->n_targets, H, W);
    table_morph(t, h->morph, h->n_morph);                   // (check_morph_list passed)
    return t;
}
TargetTable default_targets(int H, int W) { return target_table(&kDefaultTarget, 1, H, W); }

int ensure_tail_buffers(mi_unet *h, size_t ws_bytes, size_t plane_bytes)
{
    if (ws_bytes <= h->tail_ws_bytes && plane_bytes <= h->multi_cap) return 0;
    if (h->tail_stream) HIP_TRY(hipStreamSynchronize(h->tail_stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
    if (ws_bytes > h->tail_ws_bytes) {
        h->tail_ws_bytes = 0;
        HIP_TRY(h->d_tail_ws.reset(ws_bytes));
        h->tail_ws_bytes = ws_bytes;
    }
    if (plane_bytes > h->multi_cap) {
        h->multi_cap = 0;
        HIP_TRY(h->d_multi.reset(plane_bytes));
        for (auto &b : h->h_multi) HIP_TRY(b.reset(plane_bytes));
        h->multi_cap = plane_bytes;
    }
    return 0;
}

int infer_microbatch(mi_unet *h, const uint8_t *d_imgs, int B, uint8_t *d_labels, float *d_logits)
{
    if (int rc = run_microbatch(h, d_imgs, B, d_labels, d_logits)) return rc;
    return h->postprocess ? device_postprocess(h, d_labels, B) : 0;
}

int check_handle(mi_unet *h, bool need_weights)
{
    if (!h) return fail(MI_UNET_EARG, "null engine handle");
    if (need_weights && !h->weights_loaded) return fail(MI_UNET_ESTATE, "Engine not initialized: load weights before inference");
    return 0;
}

DeviceWeights::~DeviceWeights()
{
    if (d) {
        int cur = 0;
        const bool have = hipGetDevice(&cur) == hipSuccess;
        (void)hipSetDevice(device);
        (void)hipFree(d);
        if (have) (void)hipSetDevice(cur);
    }
}

Routing Routing::from_env()
{
    Routing r;
    auto num = [](const char *name, int fallback) { const char *e = getenv(name); return e ? atoi(e) : fallback; };
    r.lp2 = num("MIUNET_LP2", 1);
    r.lpr = num("MIUNET_LPR", 1);
    r.lprk = num("MIUNET_LPRK", 1);
    r.convt_lpr = num("MIUNET_CONVT_LPR", 1);
    r.wino4s = num("MIUNET_WINO4S", 1);
    r.wino4_asm = num("MIUNET_WINO4_ASM", 1);
    r.fuse_first = num("MIUNET_FUSE_FIRST", 1);
    r.convt_small = num("MIUNET_CONVT_SMALL", 1) != 0;
    r.first_mfma = num("MIUNET_FIRST_MFMA", 1) != 0;
    int dev = 0;
    hipDeviceProp_t p;
    if (hipGetDevice(&dev) == hipSuccess && hipGetDeviceProperties(&p, dev) == hipSuccess && p.multiProcessorCount > 0)
        r.cus = p.multiProcessorCount;
    r.cus = persistent_cus(r.cus, getenv("MIUNET_CUS"));      // (tests: a smaller persistent grid, never below one slot per XCD)
    return r;
}

int engine_adopt_weights(mi_unet_t *h, const HostWeights &hw, bool upload)
{
    if (int rc = check_handle(h, false)) return rc;
    HIP_TRY(hipSetDevice(h->cfg.device));
    HIP_TRY(hipStreamSynchronize(h->stream));
    h->graphs.clear();                                   // (GraphRetire: also waits for the streams the handle has left)
    h->weights_loaded = false;
    h->weights.reset();
    h->d_weights = nullptr;
    auto dw = std::make_shared<DeviceWeights>();
    dw->device = h->cfg.device;
    dw->floats = hw.blob.size();
    HIP_TRY(hipMalloc(&dw->d, sizeof(float) * hw.blob.size()));
    if (upload) HIP_TRY(hipMemcpy(dw->d, hw.blob.data(), sizeof(float) * hw.blob.size(), hipMemcpyHostToDevice));
    dw->layout.conv = hw.conv; dw->layout.convT = hw.convT; dw->layout.head = hw.head; dw->layout.up_mode = hw.up_mode;
    h->weights = dw;
    h->d_weights = dw->d;
    h->weight_floats = dw->floats;
    if (int rc = build_plan(plan_input(h), dw->layout, h->plan)) return rc;
    h->weights_loaded = true;
    return MI_UNET_OK;
}

// Numeric guard of the default plan.  F(4x4,3x3) multiplies by transform constants up to 8 and 1/24, so its rounding error
// relative to the layer's operand range is about five times F(2x2,3x3)'s (measured: 2e-5 against 4e-6 on logits of magnitude
// 4 with He-initialised weights).  The path's bar is ABSOLUTE (logits within 1e-3 of the fp32 reference), so whether F(4x4)
// holds it depends on the dynamic range of the weights that were just loaded -- which only the weights can tell.  Two probe
// tiles (seeded bytes and a structured one, the engine's own size, batch 1) go through the plan twice each, every 3x3 layer on F(4x4) and every 3x3
// layer on F(2x2); if the logits differ by more than half the bar (5e-4), this weight set runs F(2x2) everywhere.  The
// difference of the two plans overstates F(4x4)'s own error (both errors add: measured 3.7e-4 apart where F(4x4) sat 2.8e-4
// from the fp32 oracle, tests/test_gpu_numeric_range.py), so a weight set that passes is inside the bar with margin.
// MIUNET_WINO4_GUARD=0 skips the probe (F(4x4) kept unconditionally), =2 trips it unconditionally, =3 probes with the noise
// tile only (tests).
static int run_numeric_guard(mi_unet_t *h)
{
    h->wino4_guard_tripped = false;
    h->guard_diff = -1.f;
    const char *ge = getenv("MIUNET_WINO4_GUARD");
    const int mode = ge ? atoi(ge) : 1;
    bool any4 = false;
    for (const Step &st : h->plan) any4 = any4 || (st.kind == Step::CONV && st.a.wpk4 != nullptr);
    if (h->algo != MI_UNET_CONV_WINOGRAD || !any4) {
        h->guard_text = "numeric guard: not applicable (this plan has no F(4x4,3x3) layer)";
        return MI_UNET_OK;
    }
    if (mode == 0) { h->guard_text = "numeric guard: skipped (MIUNET_WINO4_GUARD=0), F(4x4,3x3) kept"; return MI_UNET_OK; }
    if (mode == 2) { h->wino4_guard_tripped = true; h->guard_text = "numeric guard: tripped by MIUNET_WINO4_GUARD=2, every 3x3 layer on F(2x2,3x3)"; return MI_UNET_OK; }
    HIP_TRY(hipSetDevice(h->cfg.device));
    const int PH = h->cfg.height, PW = h->cfg.width, PC = h->cfg.in_ch;
    const size_t hw = (size_t)PH * PW, n_in = hw * PC, n_lg = hw * h->cfg.classes;
    // Two probe tiles (round 4).  (a) seeded bytes over the whole 0..255 range: every frequency, but white noise UNDER-drives a
    // trained network -- a 3x3 sum of independent bytes concentrates around its mean, and on the bench's own weights the probe
    // saw a logit range of 0.85 where structured images reach 4.  (b) a structured tile: a full-range horizontal ramp under four
    // soft ellipses of alternating sign plus three bits of noise -- large flat regions at both ends of the range, edges between
    // them (what miunet/synth.py's "blobs" images and real detector tiles look like).  The decision takes the LARGER difference.
    std::vector<uint8_t> probes[2] = { std::vector<uint8_t>(n_in), std::vector<uint8_t>(n_in) };
    uint32_t x = 0x9E3779B9u;
    for (size_t i = 0; i < n_in; ++i) { x = x * 1664525u + 1013904223u; probes[0][i] = (uint8_t)(x >> 24); }
    {
        static const float cx[4] = { 0.30f, 0.72f, 0.38f, 0.80f }, cy[4] = { 0.28f, 0.40f, 0.74f, 0.82f };
        static const float rx[4] = { 0.22f, 0.16f, 0.25f, 0.12f }, ry[4] = { 0.18f, 0.24f, 0.14f, 0.12f };
        static const float amp[4] = { 150.f, -170.f, 130.f, -200.f };
        for (int y = 0; y < PH; ++y)
            for (int xx = 0; xx < PW; ++xx) {
                float v = 255.f * (float)xx / (float)(PW > 1 ? PW - 1 : 1);
                for (int k = 0; k < 4; ++k) {
                    const float dx = ((float)xx / PW - cx[k]) / rx[k], dy = ((float)y / PH - cy[k]) / ry[k];
                    const float d = dx * dx + dy * dy;
                    v += amp[k] / (1.f + d * d * d);
                }
                x = x * 1664525u + 1013904223u;
                v += (float)(x >> 29);
                const uint8_t b = (uint8_t)(v < 0.f ? 0.f : v > 255.f ? 255.f : v);
                for (int c = 0; c < PC; ++c) probes[1][((size_t)y * PW + xx) * PC + c] = b;
            }
    }
    std::vector<float> lg4(n_lg), lg2(n_lg);
    const int keep_min = h->wino4_min_wg;
    float diff = 0.f, range = 0.f, diffs[2] = { 0.f, 0.f };
    bool finite = true;
    const int n_probes = mode == 3 ? 1 : 2;             // MIUNET_WINO4_GUARD=3: the noise tile alone (round 3's guard; tests)
    for (int pi = 0; pi < n_probes; ++pi) {
        HIP_TRY(hipStreamSynchronize(h->stream));
        HIP_TRY(hipMemcpy(h->d_img, probes[pi].data(), n_in, hipMemcpyHostToDevice));
        int rc = 0;
        h->wino4_min_wg = 0;                            // every packed layer on F(4x4), whatever its grid
        rc = launch_plan(h, h->d_img, 1, h->d_labels, h->d_logits);
        if (!rc && hipStreamSynchronize(h->stream) != hipSuccess) rc = fail(MI_UNET_EHIP, "numeric guard: probe pass failed");
        if (!rc && hipMemcpy(lg4.data(), h->d_logits, sizeof(float) * n_lg, hipMemcpyDeviceToHost) != hipSuccess) rc = fail(MI_UNET_EHIP, "numeric guard: D2H failed");
        if (!rc) {
            h->wino4_guard_tripped = true;              // the same plan with every 3x3 layer on F(2x2)
            rc = launch_plan(h, h->d_img, 1, h->d_labels, h->d_logits);
            h->wino4_guard_tripped = false;
            if (!rc && hipStreamSynchronize(h->stream) != hipSuccess) rc = fail(MI_UNET_EHIP, "numeric guard: probe pass failed");
            if (!rc && hipMemcpy(lg2.data(), h->d_logits, sizeof(float) * n_lg, hipMemcpyDeviceToHost) != hipSuccess) rc = fail(MI_UNET_EHIP, "numeric guard: D2H failed");
        }
        h->wino4_min_wg = keep_min;
        if (rc) return rc;
        for (size_t i = 0; i < n_lg; ++i) {
            const float d = std::fabs(lg4[i] - lg2[i]);
            if (!(d == d) || std::isinf(d)) finite = false;
            diffs[pi] = std::max(diffs[pi], d);
            range = std::max(range, std::fabs(lg2[i]));
        }
        diff = std::max(diff, diffs[pi]);
    }
    h->guard_diff = diff;
    h->wino4_guard_tripped = !finite || diff > h->guard_limit;
    char buf[384];
    snprintf(buf, sizeof buf, "numeric guard: probe logits (range %.3g) of the F(4x4,3x3) and F(2x2,3x3) plans differ by %.3g (noise tile %.3g, structured tile %.3g; limit %.3g): %s",
             range, diff, diffs[0], n_probes > 1 ? diffs[1] : -1.f, h->guard_limit, h->wino4_guard_tripped ? "F(2x2,3x3) on every 3x3 layer for this weight set" : "F(4x4,3x3) kept");
    h->guard_text = buf;
    return MI_UNET_OK;
}

int engine_calibrate(mi_unet_t *h)
{
    if (int rc = check_handle(h, true)) return rc;
    const int rc = run_numeric_guard(h);
    h->guard_text += h->asm_note;                       // (empty unless the assembly kernels were wanted and are not there)
    return rc;
}

float *engine_weight_ptr(mi_unet_t *h) { return h ? h->d_weights : nullptr; }
size_t engine_weight_floats(const mi_unet_t *h) { return h ? h->weight_floats : 0; }
int engine_algo(const mi_unet_t *h) { return h->algo; }
const mi_unet_config &engine_config(const mi_unet_t *h) { return h->cfg; }
hipStream_t engine_stream(const mi_unet_t *h) { return h->stream; }

// contour outputs of `bm` images: device -> pinned mirror (async, behind the kernels), and after the stream has been
// synchronised only what exists goes on to the caller's arrays (the capacity is mostly air: 2 x 32768 ints per image)
int grow_contour_buffers(mi_unet *h, const ContourLayout &cl)
{
    const size_t need = cl.ints();
    if (need <= h->cont_cap) return 0;
    HIP_TRY(hipStreamSynchronize(h->stream));
    h->cont_cap = 0;
    HIP_TRY(h->d_cont.reset(need));
    HIP_TRY(h->h_cont.reset(2 * need));       // two halves: see run_raw_call
    h->cont_cap = need;
    return 0;
}

int contours_to_pinned(mi_unet *h, const ContourLayout &cl, hipStream_t s, int half)
{
    // counts and starts whole (small), the points whole as well: 4 MB at 16 images rides PCIe in 0.1 ms once it is pinned
    HIP_TRY(hipMemcpyAsync(h->h_cont + half * h->cont_cap, h->d_cont, cl.ints() * sizeof(int), hipMemcpyDeviceToHost, s));
    return 0;
}

void contours_to_caller(const mi_unet *h, const ContourLayout &cl, int32_t *xy, int32_t *start, int32_t *counts, int half)
{
    const int *base = h->h_cont + half * h->cont_cap, *p_xy = cl.xy(base), *p_start = cl.start(base), *p_count = cl.count(base);
    const int cap_points = cl.cap_points, cap_contours = cl.cap_contours;
    for (int i = 0; i < cl.planes; ++i) {
        counts[i] = p_count[i];
        memcpy(start + (size_t)i * (cap_contours + 1), p_start + (size_t)i * (cap_contours + 1), sizeof(int) * (cap_contours + 1));
        if (p_count[i] > 0) {
            const int npts = p_start[(size_t)i * (cap_contours + 1) + p_count[i]];
            if (npts > 0 && npts <= cap_points)
                memcpy(xy + (size_t)i * cap_points * 2, p_xy + (size_t)i * cap_points * 2, sizeof(int) * 2 * (size_t)npts);
        }
    }
}

}  // namespace miunet

extern "C" {

const char *mi_unet_last_error(void) { return engine_last_error().c_str(); }

int mi_unet_device_count(void)
{
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

void mi_unet_default_config(mi_unet_config *cfg)
{
    if (!cfg) return;
    cfg->height = 512; cfg->width = 512; cfg->in_ch = 1; cfg->base = 64; cfg->levels = 4; cfg->classes = 3;
    cfg->max_batch = 16; cfg->device = 0; cfg->conv_algo = MI_UNET_CONV_AUTO;
}

// mi_unet_create (src == null: every switch from the environment, the assembly kernels loaded here) and the handle half of
// mi_unet_clone (the source's resolved switches and its assembly kernels, shared)
static int create_handle(const mi_unet_config *cfg, const mi_unet *src, mi_unet_t **out)
{
    const int L = cfg->levels;
    if (L < 1 || L > 6) return fail(MI_UNET_EARG, "levels must be in 1..6");
    if (cfg->height <= 0 || cfg->width <= 0 || cfg->height % (1 << L) || cfg->width % (1 << L))
        return fail(MI_UNET_EARG, "height and width must be positive multiples of 2^levels");
    if (cfg->in_ch != 1 && cfg->in_ch != 3) return fail(MI_UNET_EARG, "in_ch must be 1 or 3");
    if (cfg->base < 16 || (cfg->base & (cfg->base - 1)) || cfg->base > 256)
        return fail(MI_UNET_EARG, "base must be a power of two in 16..256");
    if (cfg->classes < 2 || cfg->classes > 6) return fail(MI_UNET_EARG, "classes must be in 2..6");
    if (cfg->max_batch < 1) return fail(MI_UNET_EARG, "max_batch must be >= 1");
    if (cfg->conv_algo < 0 || cfg->conv_algo > 5)
        return fail(MI_UNET_EARG, "conv_algo must be 0 (auto), 1 (direct), 2 (winograd), 3 (winograd16), 4 (bf16) or 5 (fp16)");
    int ndev = mi_unet_device_count();
    if (ndev <= 0) return fail(MI_UNET_ENODEVICE, "no HIP device visible: libmiunet has no CPU fallback");
    if (cfg->device < 0 || cfg->device >= ndev) return fail(MI_UNET_EARG, "device ordinal out of range");
    HIP_TRY(hipSetDevice(cfg->device));

    mi_unet *h = new mi_unet();
    h->cfg = *cfg;
    for (int i = 0; i <= L; ++i) h->ch[i] = cfg->base << i;
    {
        int algo = cfg->conv_algo;
        if (algo == MI_UNET_CONV_AUTO) {
            const char *env = getenv("MIUNET_CONV_ALGO");
            if (env && !strcmp(env, "direct")) algo = MI_UNET_CONV_DIRECT;
            else if (env && !strcmp(env, "winograd")) algo = MI_UNET_CONV_WINOGRAD;
            else if (env && !strcmp(env, "winograd16")) algo = MI_UNET_CONV_WINOGRAD16;
            else if (env && !strcmp(env, "bf16")) algo = MI_UNET_CONV_BF16;
            else if (env && !strcmp(env, "fp16")) algo = MI_UNET_CONV_FP16;
            else algo = MI_UNET_CONV_DEFAULT;
        }
        h->algo = algo;
        const char *gr = getenv("MIUNET_GRAPH");
        h->use_graph = !(gr && !strcmp(gr, "0"));
    }
    if (src) {                                           // a clone routes and stages exactly as its source (same device)
        h->fuse_pool = src->fuse_pool; h->fuse_head = src->fuse_head; h->wino4_min_wg = src->wino4_min_wg;
        h->routing = src->routing;
        h->asm_kernels = src->asm_kernels; h->asm_note = src->asm_note;
        h->copy_threads = src->copy_threads; h->raw_split = src->raw_split; h->raw_trace = src->raw_trace;
    } else {
        const char *fp = getenv("MIUNET_FUSE_POOL");
        h->fuse_pool = !(fp && !strcmp(fp, "0"));
        const char *fh = getenv("MIUNET_FUSE_HEAD");
        h->fuse_head = !(fh && fh[0] == '0');
        if (const char *mw = getenv("MIUNET_WINO4_MIN_WG")) h->wino4_min_wg = atoi(mw);
        h->routing = Routing::from_env();
        if (const char *ct = getenv("MIUNET_COPY_THREADS")) h->copy_threads = std::min(std::max(atoi(ct), 1), 16);
        if (const char *sp = getenv("MIUNET_RAW_SPLIT")) {
            h->raw_split.clear();
            for (const char *q = sp; *q;) {
                h->raw_split.push_back(atoi(q));
                while (*q && *q != ',') ++q;
                if (*q == ',') ++q;
            }
        }
        const char *tr = getenv("MIUNET_RAW_TRACE");
        h->raw_trace = tr && tr[0] == '1';
        // the assembly kernels' code objects, loaded before any plan is built: the routing is told here whether they are there
        if (h->algo == MI_UNET_CONV_WINOGRAD && h->routing.wino4_asm != 0) {
            h->asm_kernels = std::make_shared<AsmKernels>(cfg->device);
            if (!h->asm_kernels->available()) {
                h->asm_note = "; assembly kernels not available (" + h->asm_kernels->error() + "): their layers run conv3x3_wino4 / conv3x3_wino4s";
                h->guard_text += h->asm_note;
                h->asm_kernels.reset();
            }
        }
    }
    if (!h->asm_kernels) h->routing.wino4_asm = 0;
    auto cleanup_fail = [&](int rc) { mi_unet_destroy(h); return rc; };
#define HIP_TRY_H(expr)                                                                                        \
    do {                                                                                                       \
        hipError_t e__ = (expr);                                                                               \
        if (e__ != hipSuccess)                                                                                 \
            return cleanup_fail(fail(MI_UNET_EHIP, std::string(#expr) + ": " + hipGetErrorString(e__)));      \
    } while (0)
    HIP_TRY_H(hipStreamCreateWithFlags(&h->own_stream, hipStreamNonBlocking));
    h->stream = h->own_stream;
    HIP_TRY_H(h->tev0.reset());
    HIP_TRY_H(h->tev1.reset());
    const size_t npix0 = (size_t)cfg->max_batch * cfg->height * cfg->width;
    plan_buffer_floats(*cfg, h->cat_floats, h->s_floats);
    for (int i = 0; i < L; ++i) HIP_TRY_H(h->d_cat[i].reset(h->cat_floats[i]));
    HIP_TRY_H(h->d_s0.reset(h->s_floats));
    HIP_TRY_H(h->d_s1.reset(h->s_floats));
    HIP_TRY_H(h->d_img.reset(npix0 * cfg->in_ch));
    HIP_TRY_H(h->d_labels.reset(npix0));
    HIP_TRY_H(h->d_logits.reset(npix0 * cfg->classes));
    HIP_TRY_H(h->h_img.reset(npix0 * cfg->in_ch));
    HIP_TRY_H(h->h_labels.reset(npix0));
    {
        const char *sk = getenv("MIUNET_SPLITK");
        if (!(sk && !strcmp(sk, "0"))) {
            h->ksplit_bytes = (size_t)64 << 20;
            HIP_TRY_H(h->d_ksplit.reset(h->ksplit_bytes / sizeof(float)));
        }
    }
    HIP_TRY_H(h->d_lut.reset(256));
    float lut[256];
    first_layer_lut(lut);
    HIP_TRY_H(hipMemcpy(h->d_lut, lut, sizeof lut, hipMemcpyHostToDevice));
#undef HIP_TRY_H
    *out = h;
    return MI_UNET_OK;
}

int mi_unet_create(const mi_unet_config *cfg, mi_unet_t **out)
{
    if (!cfg || !out) return fail(MI_UNET_EARG, "mi_unet_create: null argument");
    *out = nullptr;
    return create_handle(cfg, nullptr, out);
}

int mi_unet_load_weights_from_memory(mi_unet_t *h, const void *blob, size_t len)
{
    if (int rc = check_handle(h, false)) return rc;
    if (!blob) return fail(MI_UNET_EARG, "null weight blob");
    HostWeights hw;
    if (int rc = engine_pack_weights(h->cfg, h->algo, blob, len, hw)) return rc;
    if (int rc = engine_adopt_weights(h, hw, /*upload=*/true)) return rc;
    return engine_calibrate(h);
}

int mi_unet_load_weights(mi_unet_t *h, const char *path)
{
    if (int rc = check_handle(h, false)) return rc;
    if (!path) return fail(MI_UNET_EARG, "null weight path");
    std::ifstream f(path, std::ios::binary | std::ios::ate);
    if (!f.good()) return fail(MI_UNET_EFILE, std::string("Engine file not found: ") + path);
    const std::streamsize sz = f.tellg();
    f.seekg(0);
    std::vector<char> buf((size_t)sz);
    if (!f.read(buf.data(), sz)) return fail(MI_UNET_EFILE, std::string("cannot read ") + path);
    return mi_unet_load_weights_from_memory(h, buf.data(), buf.size());
}

int mi_unet_clone(const mi_unet_t *src, int max_batch, mi_unet_t **out)
{
    if (!src || !out) return fail(MI_UNET_EARG, "mi_unet_clone: null argument");
    *out = nullptr;
    if (!src->weights_loaded || !src->weights) return fail(MI_UNET_ESTATE, "mi_unet_clone: the source engine has no weights yet");
    mi_unet_config cfg = src->cfg;
    if (max_batch > 0) cfg.max_batch = max_batch;
    cfg.conv_algo = src->algo;                       // the resolved algorithm: the shared blob is packed for it
    mi_unet_t *h = nullptr;
    if (int rc = create_handle(&cfg, src, &h)) return rc;
    h->wino4_guard_tripped = src->wino4_guard_tripped; h->guard_diff = src->guard_diff; h->guard_text = src->guard_text;
    h->weights = src->weights;                       // shared: freed with the last handle that holds it
    h->d_weights = h->weights->d;
    h->weight_floats = h->weights->floats;
    if (int rc = build_plan(plan_input(h), h->weights->layout, h->plan)) { mi_unet_destroy(h); return rc; }
    h->weights_loaded = true;
    *out = h;
    return MI_UNET_OK;
}

int mi_unet_infer_u8_device(mi_unet_t *h, const uint8_t *d_imgs, int B, uint8_t *d_labels, float *d_logits)
{
    if (int rc = check_handle(h, true)) return rc;
    if (!d_imgs || !d_labels || B < 0) return fail(MI_UNET_EARG, "mi_unet_infer_u8_device: bad argument");
    HIP_TRY(hipSetDevice(h->cfg.device));
    const size_t hw = (size_t)h->cfg.height * h->cfg.width;
    for (int b0 = 0; b0 < B; b0 += h->cfg.max_batch) {
        const int bm = (B - b0) < h->cfg.max_batch ? (B - b0) : h->cfg.max_batch;
        if (int rc = infer_microbatch(h, d_imgs + b0 * hw * h->cfg.in_ch, bm, d_labels + b0 * hw,
                                      d_logits ? d_logits + b0 * hw * h->cfg.classes : nullptr))
            return rc;
    }
    return MI_UNET_OK;
}

int mi_unet_infer_u8(mi_unet_t *h, const uint8_t *imgs, int B, uint8_t *labels, float *logits)
{
    if (int rc = check_handle(h, true)) return rc;
    if (!imgs || !labels || B < 0) return fail(MI_UNET_EARG, "mi_unet_infer_u8: bad argument");
    HIP_TRY(hipSetDevice(h->cfg.device));
    const size_t hw = (size_t)h->cfg.height * h->cfg.width;
    hipStream_t s = h->stream;
    for (int b0 = 0; b0 < B; b0 += h->cfg.max_batch) {
        const int bm = (B - b0) < h->cfg.max_batch ? (B - b0) : h->cfg.max_batch;
        const size_t in_bytes = bm * hw * h->cfg.in_ch;
        memcpy(h->h_img, imgs + b0 * hw * h->cfg.in_ch, in_bytes);
        HIP_TRY(hipMemcpyAsync(h->d_img, h->h_img, in_bytes, hipMemcpyHostToDevice, s));
        if (int rc = infer_microbatch(h, h->d_img, bm, h->d_labels, logits ? h->d_logits : nullptr)) return rc;
        HIP_TRY(hipMemcpyAsync(h->h_labels, h->d_labels, bm * hw, hipMemcpyDeviceToHost, s));
        if (logits)
            HIP_TRY(hipMemcpyAsync(logits + b0 * hw * h->cfg.classes, h->d_logits, sizeof(float) * bm * hw * h->cfg.classes,
                                   hipMemcpyDeviceToHost, s));
        HIP_TRY(hipStreamSynchronize(s));
        memcpy(labels + b0 * hw, h->h_labels, bm * hw);
    }
    return MI_UNET_OK;
}

int mi_unet_set_postprocess(mi_unet_t *h, int on)
{
    if (int rc = check_handle(h, false)) return rc;
    h->postprocess = on != 0;
    return MI_UNET_OK;
}

int mi_unet_target_min_area(int H, int W, float frac) { return static_cast<int>(W * H * frac); }

int mi_unet_set_targets(mi_unet_t *h, const mi_unet_target *t, int n)
{
    if (int rc = check_handle(h, false)) return rc;
    if (n < 0 || n > MI_UNET_MAX_TARGETS)
        return fail(MI_UNET_EARG, "mi_unet_set_targets: " + std::to_string(n) + " targets (at most " + std::to_string(MI_UNET_MAX_TARGETS) + ")");
    if (!t || n == 0) { t = &kDefaultTarget; n = 1; }
    for (int k = 0; k < n; ++k) {
        if (t[k].cls < 1 || t[k].cls >= h->cfg.classes)
            return fail(MI_UNET_EARG, "mi_unet_set_targets: class " + std::to_string(t[k].cls) + " is outside 1.." + std::to_string(h->cfg.classes - 1));
        for (int j = 0; j < k; ++j)
            if (t[j].cls == t[k].cls) return fail(MI_UNET_EARG, "mi_unet_set_targets: class " + std::to_string(t[k].cls) + " is listed twice");
        if (!(std::isfinite(t[k].min_area_frac) && t[k].min_area_frac >= 0.f && t[k].min_area_frac <= 1.f))
            return fail(MI_UNET_EARG, "mi_unet_set_targets: min_area_frac of class " + std::to_string(t[k].cls) + " must be finite and in [0, 1]");
    }
    mi_unet_target keep[MI_UNET_MAX_TARGETS];        // (t may point into h->targets)
    std::copy(t, t + n, keep);
    std::copy(keep, keep + n, h->targets);
    h->n_targets = n;
    return MI_UNET_OK;
}

int mi_unet_get_targets(const mi_unet_t *h, mi_unet_target *t, int cap, int *n)
{
    if (!h || !n || cap < 0 || (cap > 0 && !t)) return fail(MI_UNET_EARG, "mi_unet_get_targets: bad argument");
    *n = h->n_targets;
    for (int k = 0; k < h->n_targets && k < cap; ++k) t[k] = h->targets[k];
    return MI_UNET_OK;
}

int mi_unet_set_morph(mi_unet_t *h, const mi_unet_morph *m, int n)
{
    if (int rc = check_handle(h, false)) return rc;
    if (n < 0 || n > MI_UNET_MAX_TARGETS)
        return fail(MI_UNET_EARG, "mi_unet_set_morph: " + std::to_string(n) + " entries (at most " + std::to_string(MI_UNET_MAX_TARGETS) + ")");
    if (!m || n == 0) { m = &kDefaultMorph; n = 1; }
    for (int k = 0; k < n; ++k) {
        if (m[k].shape != MI_UNET_MORPH_RECT && m[k].shape != MI_UNET_MORPH_DISC)
            return fail(MI_UNET_EARG, "mi_unet_set_morph: unknown shape " + std::to_string(m[k].shape));
        if (m[k].open_r < 0 || m[k].open_r > MI_UNET_MORPH_MAX_R || m[k].close_r < 0 || m[k].close_r > MI_UNET_MORPH_MAX_R)
            return fail(MI_UNET_EARG, "mi_unet_set_morph: radius outside 0.." + std::to_string(MI_UNET_MORPH_MAX_R));
    }
    mi_unet_morph keep[MI_UNET_MAX_TARGETS];           // (m may point into h->morph)
    std::copy(m, m + n, keep);
    std::copy(keep, keep + n, h->morph);
    h->n_morph = n;
    return MI_UNET_OK;
}

int mi_unet_get_morph(const mi_unet_t *h, mi_unet_morph *m, int cap, int *n)
{
    if (!h || !n || cap < 0 || (cap > 0 && !m)) return fail(MI_UNET_EARG, "mi_unet_get_morph: bad argument");
    *n = h->n_morph;
    for (int k = 0; k < h->n_morph && k < cap; ++k) m[k] = h->morph[k];
    return MI_UNET_OK;
}

int mi_unet_morph_element(int shape, int r, uint8_t *elem)
{
    if (!elem || (shape != MI_UNET_MORPH_RECT && shape != MI_UNET_MORPH_DISC) || r < 0 || r > MI_UNET_MORPH_MAX_R)
        return fail(MI_UNET_EARG, "mi_unet_morph_element: bad argument");
    for (int dy = -r; dy <= r; ++dy)
        for (int dx = -r; dx <= r; ++dx)
            elem[(dy + r) * (2 * r + 1) + dx + r] = shape == MI_UNET_MORPH_RECT || dx * dx + dy * dy <= r * r;
    return MI_UNET_OK;
}

// mi_unet_postprocess_masks and its _multi form: label maps up, the chain per micro-batch, masks down.  The first runs the reference's
// target in place in the network's scratch buffer (device_postprocess), _multi the handle's K targets into d_multi on the tail workspace.
static int postprocess_masks_call(mi_unet_t *h, const char *fn, bool multi, const uint8_t *labels, int B, uint8_t *out)
{
    if (int rc = check_handle(h, false)) return rc;
    if (!labels || !out || B < 0) return fail(MI_UNET_EARG, std::string(fn) + ": bad argument");
    HIP_TRY(hipSetDevice(h->cfg.device));
    const int H = h->cfg.height, W = h->cfg.width, Bm = h->cfg.max_batch;
    const size_t hw = (size_t)H * W;
    if (multi)
        if (int rc = check_morph_list(h, fn)) return rc;
    const TargetTable tab = multi ? target_table(h, H, W) : default_targets(H, W);
    const size_t K = (size_t)tab.K;
    if (multi && (size_t)std::min(B, Bm) * K * hw > 0x7FFFFFFFull)
        return fail(MI_UNET_EARG, std::string(fn) + ": max_batch x targets x height x width exceeds 2^31 - 1");
    hipStream_t s = h->stream;
    for (int b0 = 0; b0 < B; b0 += Bm) {
        const int bm = std::min(Bm, B - b0);
        if (multi)
            if (int rc = ensure_tail_buffers(h, postprocess_workspace_bytes(bm * tab.K, H, W), bm * K * hw)) return rc;
        uint8_t *const d_out = multi ? h->d_multi.get() : h->d_labels.get(), *const h_out = multi ? h->h_multi[0].get() : h->h_labels.get();
        memcpy(h->h_labels, labels + b0 * hw, bm * hw);
        HIP_TRY(hipMemcpyAsync(h->d_labels, h->h_labels, bm * hw, hipMemcpyHostToDevice, s));
        if (int rc = multi ? enqueue_tail(h, h->d_labels, bm, H, W, tab, d_out, h->d_tail_ws, nullptr, nullptr, s)
                           : device_postprocess(h, h->d_labels, bm))
            return rc;
        HIP_TRY(hipMemcpyAsync(h_out, d_out, bm * K * hw, hipMemcpyDeviceToHost, s));
        HIP_TRY(hipStreamSynchronize(s));
        memcpy(out + b0 * K * hw, h_out, bm * K * hw);
    }
    return MI_UNET_OK;
}

int mi_unet_postprocess_masks(mi_unet_t *h, const uint8_t *labels, int B, uint8_t *out)
{
    return postprocess_masks_call(h, "mi_unet_postprocess_masks", false, labels, B, out);
}

int mi_unet_postprocess_masks_multi(mi_unet_t *h, const uint8_t *labels, int B, uint8_t *out)
{
    return postprocess_masks_call(h, "mi_unet_postprocess_masks_multi", true, labels, B, out);
}

int mi_unet_extract_contours(mi_unet_t *h, const uint8_t *masks, int B, int32_t *xy, int cap_points, int32_t *start,
                             int cap_contours, int32_t *counts)
{
    if (int rc = check_handle(h, false)) return rc;
    if (!masks || !xy || !start || !counts || B < 0 || cap_points <= 0 || cap_contours <= 0)
        return fail(MI_UNET_EARG, "mi_unet_extract_contours: bad argument");
    HIP_TRY(hipSetDevice(h->cfg.device));
    const int H = h->cfg.height, W = h->cfg.width;
    const size_t hw = (size_t)H * W;
    const size_t scratch = sizeof(float) * (size_t)h->cfg.max_batch * hw * h->ch[0];
    hipStream_t s = h->stream;
    for (int b0 = 0; b0 < B; b0 += h->cfg.max_batch) {
        const int bm = (B - b0) < h->cfg.max_batch ? (B - b0) : h->cfg.max_batch;
        if (contour_workspace_bytes(bm, H, W, cap_contours) > scratch)
            return fail(MI_UNET_EARG, "contour workspace does not fit the scratch buffer (cap_contours too large)");
        const ContourLayout cl{ bm, cap_points, cap_contours };
        if (int rc = grow_contour_buffers(h, cl)) return rc;
        int *const d_cont = h->d_cont;
        memcpy(h->h_labels, masks + b0 * hw, bm * hw);
        HIP_TRY(hipMemcpyAsync(h->d_labels, h->h_labels, bm * hw, hipMemcpyHostToDevice, s));
        const hipError_t e = launch_extract_contours(h->d_labels, bm, H, W, cl.xy(d_cont), cap_points, cl.start(d_cont), cap_contours, cl.count(d_cont), h->d_s1, s);
        if (e != hipSuccess) return fail(MI_UNET_EHIP, std::string("contour launch: ") + hipGetErrorString(e));
        if (int rc = contours_to_pinned(h, cl, s)) return rc;
        HIP_TRY(hipStreamSynchronize(s));
        contours_to_caller(h, cl, xy + (size_t)b0 * cap_points * 2, start + (size_t)b0 * (cap_contours + 1), counts + b0);
    }
    return MI_UNET_OK;
}

int mi_unet_host_alloc(size_t bytes, void **p)
{
    if (!p || bytes == 0) return fail(MI_UNET_EARG, "mi_unet_host_alloc: bad argument");
    *p = nullptr;
    if (mi_unet_device_count() <= 0) return fail(MI_UNET_ENODEVICE, "no HIP device visible: libmiunet has no CPU fallback");
    HIP_TRY(hipHostMalloc(p, bytes, hipHostMallocDefault));
    return MI_UNET_OK;
}

void mi_unet_host_free(void *p)
{
    if (p) (void)hipHostFree(p);
}

int mi_unet_set_stream(mi_unet_t *h, void *hip_stream)
{
    if (int rc = check_handle(h, false)) return rc;
    hipStream_t next = hip_stream ? static_cast<hipStream_t>(hip_stream) : h->own_stream;
    if (next == h->stream) return MI_UNET_OK;
    // Leaving a caller's stream on which cached graphs may still be replaying: an event behind them, for GraphRetire.  (The handle's
    // own stream outlives its entries and is waited for directly.)  Nothing waits here: the caller orders the switch.
    if (h->stream != h->own_stream && h->graphs.holds_stream(h->stream)) {
        HIP_TRY(hipSetDevice(h->cfg.device));
        auto &ls = h->left_streams;
        ls.erase(std::remove_if(ls.begin(), ls.end(), [h](const mi_unet::LeftStream &l) { return !h->graphs.holds_stream(l.stream); }), ls.end());
        auto it = std::find_if(ls.begin(), ls.end(), [h](const mi_unet::LeftStream &l) { return l.stream == h->stream; });
        if (it == ls.end()) {
            ls.emplace_back();
            it = ls.end() - 1;
            it->stream = h->stream;
            const hipError_t e = it->done.reset(hipEventDisableTiming);
            if (e != hipSuccess) { ls.pop_back(); return fail(MI_UNET_EHIP, std::string("mi_unet_set_stream: hipEventCreate: ") + hipGetErrorString(e)); }
        }
        HIP_TRY(hipEventRecord(it->done, h->stream));
    }
    h->stream = next;
    return MI_UNET_OK;
}

int mi_unet_sync(mi_unet_t *h)
{
    if (int rc = check_handle(h, false)) return rc;
    HIP_TRY(hipStreamSynchronize(h->stream));
    return MI_UNET_OK;
}

int mi_unet_timer_begin(mi_unet_t *h)
{
    if (int rc = check_handle(h, false)) return rc;
    HIP_TRY(hipEventRecord(h->tev0, h->stream));
    return MI_UNET_OK;
}

int mi_unet_timer_end(mi_unet_t *h, float *ms)
{
    if (int rc = check_handle(h, false)) return rc;
    if (!ms) return fail(MI_UNET_EARG, "null ms");
    HIP_TRY(hipEventRecord(h->tev1, h->stream));
    HIP_TRY(hipEventSynchronize(h->tev1));
    HIP_TRY(hipEventElapsedTime(ms, h->tev0, h->tev1));
    return MI_UNET_OK;
}

int mi_unet_set_profiling(mi_unet_t *h, int on)
{
    if (int rc = check_handle(h, false)) return rc;
    h->profiling = on != 0;
    h->stats.clear();
    h->ev_used = 0;
    return MI_UNET_OK;
}

int mi_unet_get_kernel_stats(mi_unet_t *h, mi_unet_kernel_stat *stats, int cap, int *n)
{
    if (int rc = check_handle(h, false)) return rc;
    if (!n) return fail(MI_UNET_EARG, "null n");
    *n = (int)h->stats.size();
    if (!h->stats.empty()) HIP_TRY(hipEventSynchronize(h->ev_pool[2 * h->stats.size() - 1]));
    for (size_t i = 0; i < h->stats.size(); ++i)
        if (h->stats[i].ms < 0.f) HIP_TRY(hipEventElapsedTime(&h->stats[i].ms, h->ev_pool[2 * i], h->ev_pool[2 * i + 1]));
    for (int i = 0; i < *n && i < cap && stats; ++i) stats[i] = h->stats[i];
    return MI_UNET_OK;
}

const char *mi_unet_numeric_guard(const mi_unet_t *h, int *tripped, float *diff)
{
    if (!h) return "";
    if (tripped) *tripped = h->wino4_guard_tripped ? 1 : 0;
    if (diff) *diff = h->guard_diff;
    return h->guard_text.c_str();
}

// The handle's buffers and events free themselves (engine_handle.h); what is left has an order: no stream the handle launched on
// may still be working when they go, and the graph executables go before the stream they were captured on and before the assembly
// kernels' modules, which the last handle that shares them unloads.
void mi_unet_destroy(mi_unet_t *h)
{
    if (!h) return;
    (void)hipSetDevice(h->cfg.device);
    for (hipStream_t q : { h->stream, h->own_stream, h->tail_stream, h->dl_stream, h->pre_stream })   // (h->stream: the caller's, after mi_unet_set_stream)
        if (q) (void)hipStreamSynchronize(q);
    for (hipStream_t q : { h->tail_stream, h->dl_stream, h->pre_stream })
        if (q) (void)hipStreamDestroy(q);
    h->graphs.clear();
    if (h->own_stream) (void)hipStreamDestroy(h->own_stream);
    delete h;                                           // ... and with it this handle's hold on the weights and the assembly kernels
}

}  // extern "C"
