// debug.cpp -- the test and diagnosis entry points: mi_unet_layer_debug (one kernel on caller-supplied operands) and its strided form
// mi_unet_layer_debug_strided (the same launch in a concat-buffer layout between poisoned guards, the raw allocations returned),
// mi_unet_debug_layer_info / mi_unet_debug_capture and the taps launch_plan calls for them.
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

using namespace miunet;

namespace {

// one image's [npix][C] tensor (pixel stride `ld` elements of `bits` bits, kind: 1 = bf16, 2 = fp16 for 16-bit storage) -> dense floats
int download_tensor(hipStream_t s, const void *d, int bits, int lp_kind, size_t npix, int C, int ld, float *dst)
{
    if (!dst) return 0;
    const size_t eb = (size_t)bits / 8;
    std::vector<unsigned char> raw(npix * C * eb);
    HIP_TRY(hipStreamSynchronize(s));
    if (ld == C) HIP_TRY(hipMemcpy(raw.data(), d, npix * C * eb, hipMemcpyDeviceToHost));
    else HIP_TRY(hipMemcpy2D(raw.data(), C * eb, d, (size_t)ld * eb, C * eb, npix, hipMemcpyDeviceToHost));
    const size_t n = npix * C;
    if (bits == 32) memcpy(dst, raw.data(), n * 4);
    else if (bits == 8) for (size_t i = 0; i < n; ++i) dst[i] = (float)raw[i];
    else {
        const uint16_t *r16 = reinterpret_cast<const uint16_t *>(raw.data());
        for (size_t i = 0; i < n; ++i) dst[i] = lp_kind == 2 ? fp16_to_float(r16[i]) : bf16_to_float(r16[i]);
    }
    return 0;
}

}  // namespace

namespace miunet {

// mi_unet_debug_capture: the tensor step `st` is about to read ...
int tap_input(mi_unet *h, const Step &st, const Launch &l, const uint8_t *d_imgs, int lp_kind)
{
    hipStream_t s = h->stream;
    const size_t im = (size_t)h->tap.img;
    const int abits = lp_kind ? 16 : 32;
    if (st.kind == Step::FIRST || (l.rc.fused & FUSE_FIRST)) {
        // (a step that runs the first layer in its loader reads the u8 image: that is what the caller's `in` buffer receives)
        const Step &f = h->plan[0];
        h->tap.info->in_bits = 8;
        h->tap.info->fused_first = st.kind != Step::FIRST;
        return download_tensor(s, d_imgs + im * f.H * f.W * f.C, 8, 0, (size_t)f.H * f.W, f.C, f.C, h->tap.in);
    }
    if (st.kind == Step::CONV || st.kind == Step::CONVT) {
        h->tap.info->in_bits = abits;
        const size_t npix = (size_t)st.a.H * st.a.W;
        return download_tensor(s, reinterpret_cast<const char *>(st.a.in) + im * npix * st.a.ldc * (abits / 8), abits, lp_kind, npix, st.a.Cin,
                               st.a.ldc, h->tap.in);
    }
    const int b = st.kind == Step::HEAD ? 32 : abits;           // POOL, UPSAMPLE (activation type), HEAD (always fp32)
    h->tap.info->in_bits = b;
    const size_t npix = (size_t)st.H * st.W;
    const int ld = (st.kind == Step::HEAD || st.kind == Step::UPSAMPLE) ? st.C : st.ld;
    return download_tensor(s, reinterpret_cast<const char *>(st.src) + im * npix * ld * (b / 8), b, lp_kind, npix, st.C, ld, h->tap.in);
}

// ... and what it stored
int tap_output(mi_unet *h, const Step &st, const Launch &l, uint8_t *d_labels, float *d_logits, int lp_kind)
{
    hipStream_t s = h->stream;
    mi_unet_layer_info *ti = h->tap.info;
    snprintf(ti->kernel, sizeof ti->kernel, "%s", route_name(l.rc.route, l.rc.fused).c_str());
    const size_t im = (size_t)h->tap.img;
    const int abits = lp_kind ? 16 : 32;
    const ConvArgs &ta = l.a;
    if (st.kind == Step::HEAD || (l.rc.fused & FUSE_HEAD)) {
        const size_t hw = (size_t)h->cfg.height * h->cfg.width;
        const int classes = h->cfg.classes;
        ti->fused_head = st.kind == Step::CONV;
        ti->out_bits = 32;
        if (d_logits)
            if (int rc = download_tensor(s, d_logits + im * classes * hw, 32, 0, classes * hw, 1, 1, h->tap.out)) return rc;
        if (h->tap.labels) {
            HIP_TRY(hipStreamSynchronize(s));
            HIP_TRY(hipMemcpy(h->tap.labels, d_labels + im * hw, hw, hipMemcpyDeviceToHost));
        }
        return 0;
    }
    if (st.kind == Step::FIRST) {
        ti->out_bits = abits;
        const size_t npix = (size_t)st.H * st.W;
        return download_tensor(s, reinterpret_cast<const char *>(st.dst) + im * npix * st.ld * (abits / 8), abits, lp_kind, npix, st.Cout, st.ld, h->tap.out);
    }
    if (st.kind == Step::CONV || st.kind == Step::CONVT) {
        const int ob = (lp_kind && ta.out_lp) ? 16 : 32;
        ti->out_bits = ob;
        const size_t npix = (size_t)ta.H * ta.W * (st.kind == Step::CONVT ? 4 : 1);
        if (int rc = download_tensor(s, reinterpret_cast<const char *>(ta.out) + (im * npix * ta.ldo + ta.co_off) * (ob / 8), ob, lp_kind, npix, ta.Cout,
                                     ta.ldo, h->tap.out))
            return rc;
        if (st.kind == Step::CONV && ta.pool_out) {
            ti->pooled = 1;
            return download_tensor(s, reinterpret_cast<const char *>(ta.pool_out) + im * (npix / 4) * ta.pool_ld * (ob / 8), ob, lp_kind, npix / 4,
                                   ta.Cout, ta.pool_ld, h->tap.pooled);
        }
        return 0;
    }
    ti->out_bits = abits;
    if (st.kind == Step::UPSAMPLE) {                             // the slice it wrote: channels [co_off, co_off + C) of the concat buffer
        const size_t npix = (size_t)(2 * st.H) * (2 * st.W);
        return download_tensor(s, reinterpret_cast<const char *>(st.dst) + (im * npix * st.ld + st.co_off) * (abits / 8), abits, lp_kind, npix, st.C,
                               st.ld, h->tap.out);
    }
    const size_t npix = (size_t)(st.H / 2) * (st.W / 2);         // POOL
    return download_tensor(s, reinterpret_cast<const char *>(st.dst) + im * npix * st.C * (abits / 8), abits, lp_kind, npix, st.C, st.C, h->tap.out);
}

}  // namespace miunet

namespace {

// mi_unet_layer_debug's ops: each runs one route -- or, for "conv3x3_wino4", the F(4x4,3x3) family as route_wino4 picks it --
// on weights packed for it.  lp: the operands are 0 fp32, 1 bf16, 2 fp16.
struct DebugOp { const char *op; Route route; Pack pack; int lp; bool routed; };
const DebugOp kDebugOps[] = {
    { "conv3x3", Route::CONV_MFMA, Pack::MFMA, 0, false },         { "convT2x2", Route::CONVT_MFMA, Pack::MFMA_T, 0, false },
    { "convT2x2_taps", Route::CONVT_TAPS, Pack::TAPS, 0, false },   { "conv3x3_wino", Route::CONV_WINO, Pack::WINO, 0, false },
    { "conv3x3_wino16", Route::CONV_WINO16, Pack::WINO16, 0, false }, { "conv3x3_wino4", Route::CONV_WINO4, Pack::WINO4, 0, true },
    { "conv3x3_wino4s", Route::CONV_WINO4S, Pack::WINO4, 0, false }, { "conv3x3_wino4a", Route::CONV_WINO4A, Pack::WINO4, 0, false },
    { "conv3x3_wino4b", Route::CONV_WINO4B, Pack::WINO4, 0, false },
    { "conv3x3_bf16", Route::CONV_BF16, Pack::LP, 1, false },       { "conv3x3_fp16", Route::CONV_FP16, Pack::LP, 2, false },
    { "conv3x3_bf16w", Route::CONV_BF16W, Pack::LP, 1, false },     { "conv3x3_fp16w", Route::CONV_FP16W, Pack::LP, 2, false },
    { "conv3x3_bf16r", Route::CONV_BF16R, Pack::LP, 1, false },     { "conv3x3_fp16r", Route::CONV_FP16R, Pack::LP, 2, false },
    { "conv3x3_bf16k", Route::CONV_BF16K, Pack::LP, 1, false },     { "conv3x3_fp16k", Route::CONV_FP16K, Pack::LP, 2, false },
    { "convT2x2_bf16", Route::CONVT_BF16, Pack::LP_T, 1, false },   { "convT2x2_fp16", Route::CONVT_FP16, Pack::LP_T, 2, false },
    { "convT2x2_bf16r", Route::CONVT_BF16R, Pack::LP_T, 1, false }, { "convT2x2_fp16r", Route::CONVT_FP16R, Pack::LP_T, 2, false },
    { "conv3x3_first", Route::FIRST, Pack::FIRST, 0, false },        { "conv3x3_first_bf16", Route::FIRST, Pack::FIRST, 1, false },
    { "conv3x3_first_fp16", Route::FIRST, Pack::FIRST, 2, false },   { "maxpool", Route::POOL, Pack::NONE, 0, false },
    { "upsample2x", Route::UPSAMPLE, Pack::UP, 0, false },           { "upsample2x_bf16", Route::UPSAMPLE, Pack::UP, 1, false },
    { "upsample2x_fp16", Route::UPSAMPLE, Pack::UP, 2, false },
    { "maxpool_bf16", Route::POOL, Pack::NONE, 1, false },           { "maxpool_fp16", Route::POOL, Pack::NONE, 2, false },
};

// The layout of one hook call, in elements (0 = the dense default), and the guard in front of and behind every device tensor
struct DebugLayout { int ldc = 0, ldo = 0, co_off = 0, pool_ld = 0; size_t guard = 0; };

// What the one body leaves behind for its two callers: the output (and pooled) allocations, guards included, still on the device
struct DebugRun {
    DeviceBuf<unsigned char> d_out, d_pool;
    size_t guard = 0, out_bytes = 0, pool_bytes = 0;             // whole allocations: guard + tensor + guard
    size_t out_npix = 0, pool_npix = 0;
    int es = 4, lp_kind = 0, C = 0, ldo = 0, co_off = 0, pool_ld = 0;
    bool pooled = false;
    std::string kernel;
};

// The body of mi_unet_layer_debug and mi_unet_layer_debug_strided: pack, upload, launch, synchronise.
int run_layer(int device, const char *op, const float *in, int B, int H, int W, int Cin, const float *w, const float *scale,
              const float *shift, int Cout, int relu, const DebugLayout &lay, DebugRun &run)
{
    if (!op || !in || B <= 0 || H <= 0 || W <= 0 || Cin <= 0) return fail(MI_UNET_EARG, "layer_debug: bad argument");
    if (mi_unet_device_count() <= 0) return fail(MI_UNET_ENODEVICE, "no HIP device visible: libmiunet has no CPU fallback");
    HIP_TRY(hipSetDevice(device));
    // ---- resolve the op: "<op>[_splitk[N]][_pool][_lpout]"; _pool returns the fused 2x2 max-pooled tensor [B][H/2][W/2][Cout] instead;
    // _splitk hands the launch a split-K workspace as the plan does (8 slabs [B][H][W][Cout], at most the engine's 64 MiB), _splitk<N>,
    // N = 2 .. 8, one of exactly N slabs (the launcher's shrink-to-fit)
    std::string o(op);
    auto strip = [&](const char *suffix) {
        const size_t n = strlen(suffix);
        if (o.size() <= n || o.compare(o.size() - n, n, suffix) != 0) return false;
        o.resize(o.size() - n);
        return true;
    };
    const bool lp_out = strip("_lpout"), want_pool = strip("_pool");
    int splitk_slabs = strip("_splitk") ? 8 : 0;
    const bool splitk_exact = splitk_slabs == 0 && o.size() > 8 && o.compare(o.size() - 8, 7, "_splitk") == 0 && o.back() >= '2' && o.back() <= '8';
    if (splitk_exact) { splitk_slabs = o.back() - '0'; o.resize(o.size() - 8); }
    if (splitk_slabs && o != "conv3x3_wino" && o != "conv3x3_wino4")
        return fail(MI_UNET_EARG, "layer_debug: _splitk is for conv3x3_wino and conv3x3_wino4");
    const DebugOp *dop = nullptr;
    for (const DebugOp &k : kDebugOps)
        if (o == k.op) dop = &k;
    if (!dop) return fail(MI_UNET_EARG, "layer_debug: unknown op " + o);
    const Pack pk = dop->pack;
    const int kind = dop->lp;                                  // operands: 0 fp32, 1 bf16, 2 fp16
    const bool up = pk == Pack::UP, first = pk == Pack::FIRST, pool = pk == Pack::NONE;
    const bool T = pk == Pack::MFMA_T || pk == Pack::TAPS || pk == Pack::LP_T;
    if (up) {
        if (Cin % 16 || want_pool || lp_out) return fail(MI_UNET_EARG, "layer_debug: upsample2x needs Cin % 16 == 0");
    } else if (first) {
        if (!w || Cout <= 0 || Cout % 4 || (Cin != 1 && Cin != 3) || want_pool || lp_out)
            return fail(MI_UNET_EARG, "layer_debug: conv3x3_first needs weights, Cin 1 or 3, Cout % 4 == 0");
    } else if (pool) {
        if (Cin % (kind ? 8 : 4) || H % 2 || W % 2 || lp_out)
            return fail(MI_UNET_EARG, "layer_debug: maxpool needs C % 4 == 0 (16-bit: C % 8 == 0) and even H, W");
    } else if (kind) {
        if (!w || Cout <= 0 || Cin % 8) return fail(MI_UNET_EARG, "layer_debug: 16-bit conv needs weights and Cin % 8 == 0");
    } else if (!w || Cout <= 0 || Cin % 4) {
        return fail(MI_UNET_EARG, "layer_debug: conv needs weights and Cin % 4 == 0");
    }
    if (lp_out && !kind) return fail(MI_UNET_EARG, "layer_debug: _lpout is for the 16-bit conv ops");
    if (want_pool && (pool || T || (H & 1) || (W & 1))) return fail(MI_UNET_EARG, "layer_debug: _pool is for the conv3x3 ops on even sizes");
    // the first layer reads the u8 image (`in` holds byte values 0..255), the 16-bit kernels 16-bit activations (rounded here, RNE);
    // the 16-bit upsample, pooling and first layer and the _lpout ops store 16 bits
    const size_t in_es = first ? 1 : kind ? 2 : 4;
    const bool out16 = kind && (up || first || pool || lp_out);
    const size_t out_es = out16 ? 2 : 4;
    const int Co = (up || pool) ? Cin : Cout;                  // channels of the output slice

    // ---- the layout: what the op has no operand for stays at its default, the rest is bounded here and by the route's launcher
    const int ldc = lay.ldc ? lay.ldc : Cin, ldo = lay.ldo ? lay.ldo : Co, co_off = lay.co_off, pool_ld = lay.pool_ld ? lay.pool_ld : Co;
    if (lay.guard % 256) return fail(MI_UNET_EARG, "layer_debug: guard_bytes must be a multiple of 256");
    if (ldc < Cin || co_off < 0 || ldo < co_off + Co || pool_ld < Co)
        return fail(MI_UNET_EARG, "layer_debug: layout needs ldc >= Cin, co_off >= 0, ldo >= co_off + Cout, pool_ld >= Cout");
    if ((first && ldc != Cin) || ((first || pool) && co_off != 0) || (pool && ldo != Co) || (!want_pool && pool_ld != Co))
        return fail(MI_UNET_EARG, "layer_debug: the op has no such stride (first layer: ldo; maxpool: ldc; pool_ld: the _pool forms)");
    const size_t in_npix = (size_t)B * H * W, in_n = in_npix * Cin;
    const size_t out_npix = (up || T) ? in_npix * 4 : pool ? in_npix / 4 : in_npix;
    const Routing rt = Routing::from_env();

    // ---- pack (weights.cpp)
    std::vector<unsigned char> in_raw(in_es == 4 ? 0 : in_n * in_es);
    for (size_t i = 0; i < in_raw.size() / in_es; ++i) {
        if (first) in_raw[i] = (uint8_t)in[i];
        else reinterpret_cast<uint16_t *>(in_raw.data())[i] = kind == 2 ? fp16_bits(in[i]) : bf16_bits(in[i]);
    }
    std::vector<float> wpk, bias;
    if (!up && !pool) {
        std::vector<double> sc(Cout, 1.0);
        bias.assign(Cout, 0.f);
        for (int co = 0; co < Cout; ++co) { bias[co] = shift ? shift[co] : 0.f; if (scale) sc[co] = scale[co]; }
        wpk.assign(packed_floats(pk, Cin, Cout), 0.f);
        pack_weights(pk, kind == 2, w, sc.data(), Cin, Cout, wpk.data());
    }
    float lut[256];
    first_layer_lut(lut);

    // ---- upload: guard + tensor + guard each.  The outputs are poisoned with NaN bytes (0xFF.. is a NaN in fp32, bf16 and fp16), so
    // that unwritten elements and stray stores are visible; so are the input's guards and its gap channels [Cin, ldc)
    const size_t G = lay.guard;
    const size_t in_bytes = in_npix * ldc * in_es, out_bytes = out_npix * ldo * out_es, pool_bytes = (out_npix / 4) * pool_ld * out_es;
    DeviceBuf<unsigned char> d_in;
    DeviceBuf<float> d_w, d_b, d_lut;
    HIP_TRY(d_in.reset(2 * G + in_bytes));
    if (G || ldc != Cin) HIP_TRY(hipMemset(d_in, 0xFF, 2 * G + in_bytes));
    const void *in_host = in_es == 4 ? static_cast<const void *>(in) : in_raw.data();
    if (ldc == Cin) HIP_TRY(hipMemcpy(d_in.get() + G, in_host, in_bytes, hipMemcpyHostToDevice));
    else HIP_TRY(hipMemcpy2D(d_in.get() + G, (size_t)ldc * in_es, in_host, Cin * in_es, Cin * in_es, in_npix, hipMemcpyHostToDevice));
    HIP_TRY(run.d_out.reset(2 * G + out_bytes));
    HIP_TRY(hipMemset(run.d_out, 0xFF, 2 * G + out_bytes));
    if (want_pool) {
        HIP_TRY(run.d_pool.reset(2 * G + pool_bytes));
        HIP_TRY(hipMemset(run.d_pool, 0xFF, 2 * G + pool_bytes));
    }
    // the split-K workspace: poisoned too, so a slab element that no slice wrote reaches the output as NaN
    DeviceBuf<unsigned char> d_ws;
    size_t ws_bytes = 0;
    if (splitk_slabs) {
        ws_bytes = (size_t)splitk_slabs * out_npix * Cout * sizeof(float);
        if (!splitk_exact && ws_bytes > ((size_t)64 << 20)) ws_bytes = (size_t)64 << 20;
        HIP_TRY(d_ws.reset(2 * G + ws_bytes));
        HIP_TRY(hipMemset(d_ws, 0xFF, 2 * G + ws_bytes));
    }
    if (!wpk.empty()) {
        HIP_TRY(d_w.reset(wpk.size()));
        HIP_TRY(d_b.reset(bias.size()));
        HIP_TRY(hipMemcpy(d_w, wpk.data(), sizeof(float) * wpk.size(), hipMemcpyHostToDevice));
        HIP_TRY(hipMemcpy(d_b, bias.data(), sizeof(float) * bias.size(), hipMemcpyHostToDevice));
    }
    if (first) {
        HIP_TRY(d_lut.reset(256));
        HIP_TRY(hipMemcpy(d_lut, lut, sizeof lut, hipMemcpyHostToDevice));
    }

    // ---- launch, synchronise
    const float *d_inf = reinterpret_cast<const float *>(d_in.get() + G);
    float *d_outf = reinterpret_cast<float *>(run.d_out.get() + G);
    Route r = dop->route;
    int ks = 1;                                               // K slices of the launch (wino4_ksplit / wino_ksplit, as the launcher asks them)
    std::unique_ptr<AsmKernels> asm_kernels;                  // no handle here: an owner for this call, when the op runs an assembly kernel
    if (up) {
        HIP_TRY(launch_upsample2x_bilinear(d_inf, ldc, d_outf, ldo, co_off, B, H, W, Cin, kind, rt, nullptr));
    } else if (first) {
        HIP_TRY(launch_conv3x3_first(d_in.get() + G, d_lut, d_w, d_b, d_outf, B, H, W, Cin, Cout, ldo, kind, rt, nullptr));
    } else if (pool) {
        if (kind) HIP_TRY(launch_maxpool2x2_u16(d_inf, ldc, d_outf, B, H, W, Cin, nullptr));
        else HIP_TRY(launch_maxpool2x2(d_inf, ldc, d_outf, B, H, W, Cin, nullptr));
    } else {
        ConvArgs a{};
        a.rt = rt;
        a.B = B; a.H = H; a.W = W; a.Cin = Cin; a.ldc = ldc; a.Cout = Cout; a.CoutPad = (int)packed_npad(pk, Cout); a.ldo = ldo; a.co_off = co_off;
        a.relu = relu;
        a.out_lp = lp_out ? 1 : 0;
        if (want_pool) { a.pool_out = reinterpret_cast<float *>(run.d_pool.get() + G); a.pool_ld = pool_ld; }
        a.in = d_inf; a.wpk = d_w; a.bias = d_b; a.out = d_outf;
        if (pk == Pack::WINO4 || pk == Pack::TAPS) a.wpk4 = d_w;
        if (splitk_slabs) { a.ksplit_ws = reinterpret_cast<float *>(d_ws.get() + G); a.ksplit_ws_bytes = ws_bytes; }      // before the routing, as plan.cpp
        if (dop->routed) r = route_wino4(a);
        if (r == Route::CONV_WINO4A || r == Route::CONV_WINO4B) {
            asm_kernels.reset(new AsmKernels(device));
            if (dop->routed && !asm_kernels->available()) {   // the routing is told, as a handle's is at create
                a.rt.wino4_asm = 0;
                r = route_wino4(a);
            }
        }
        ks = r == Route::CONV_WINO ? wino_ksplit(a) : r == Route::CONV_WINO4 ? wino4_ksplit(a, 2) : r == Route::CONV_WINO4_1B ? wino4_ksplit(a, 1) : 1;
        HIP_TRY(launch_route(r, a, asm_kernels.get(), nullptr));
    }
    HIP_TRY(hipDeviceSynchronize());
    if (splitk_slabs && G) {                                  // the workspace stays here: its guards are looked at here
        std::vector<unsigned char> g(2 * G);
        HIP_TRY(hipMemcpy(g.data(), d_ws.get(), G, hipMemcpyDeviceToHost));
        HIP_TRY(hipMemcpy(g.data() + G, d_ws.get() + G + ws_bytes, G, hipMemcpyDeviceToHost));
        for (size_t i = 0; i < 2 * G; ++i)
            if (g[i] != 0xFF)
                return fail(MI_UNET_ESTATE, "layer_debug: the launch wrote into the " + std::string(i < G ? "front" : "back") +
                                                " guard of the split-K workspace, byte " + std::to_string(i < G ? i : i - G));
    }
    run.guard = G; run.out_bytes = 2 * G + out_bytes; run.pool_bytes = want_pool ? 2 * G + pool_bytes : 0;
    run.out_npix = out_npix; run.pool_npix = out_npix / 4;
    run.es = (int)out_es; run.lp_kind = out16 ? kind : 0; run.C = Co; run.ldo = ldo; run.co_off = co_off; run.pool_ld = pool_ld;
    run.pooled = want_pool;
    run.kernel = route_name(r) + (ks > 1 ? "+splitk" + std::to_string(ks) : std::string());
    return MI_UNET_OK;
}

}  // namespace

extern "C" {

int mi_unet_layer_debug(int device, const char *op, const float *in, int B, int H, int W, int Cin, const float *w,
                        const float *scale, const float *shift, int Cout, int relu, float *out)
{
    if (!out) return fail(MI_UNET_EARG, "layer_debug: bad argument");
    DebugRun run;
    if (int rc = run_layer(device, op, in, B, H, W, Cin, w, scale, shift, Cout, relu, DebugLayout{}, run)) return rc;
    // ---- download and convert: the full-size tensor, or for _pool the pooled one
    if (run.pooled) return download_tensor(nullptr, run.d_pool.get() + run.guard, 8 * run.es, run.lp_kind, run.pool_npix, run.C, run.pool_ld, out);
    return download_tensor(nullptr, run.d_out.get() + run.guard, 8 * run.es, run.lp_kind, run.out_npix, run.C, run.ldo, out);
}

int mi_unet_layer_debug_strided(int device, const char *op, const float *in, int B, int H, int W, int Cin, const float *w,
                                const float *scale, const float *shift, int Cout, int relu, const mi_unet_debug_layout *layout,
                                void *out_raw, size_t out_cap, void *pool_raw, size_t pool_cap, mi_unet_debug_strided_info *info)
{
    if (!layout || !out_raw || !info) return fail(MI_UNET_EARG, "layer_debug_strided: null argument");
    if (layout->ldc < 0 || layout->ldo < 0 || layout->pool_ld < 0 || layout->guard_bytes < 0)
        return fail(MI_UNET_EARG, "layer_debug_strided: negative stride or guard");
    DebugLayout lay;
    lay.ldc = layout->ldc; lay.ldo = layout->ldo; lay.co_off = layout->co_off; lay.pool_ld = layout->pool_ld; lay.guard = (size_t)layout->guard_bytes;
    DebugRun run;
    if (int rc = run_layer(device, op, in, B, H, W, Cin, w, scale, shift, Cout, relu, lay, run)) return rc;
    *info = mi_unet_debug_strided_info{};
    info->elem_bytes = run.es;
    info->out_bytes = run.out_bytes;
    info->pool_bytes = run.pool_bytes;
    snprintf(info->kernel, sizeof info->kernel, "%s", run.kernel.c_str());
    if (out_cap < run.out_bytes || (run.pooled && (!pool_raw || pool_cap < run.pool_bytes)))
        return fail(MI_UNET_EARG, "layer_debug_strided: a result buffer is smaller than the allocation it receives (see info)");
    // ---- the complete allocations as they are: guards and gaps included, nothing converted
    HIP_TRY(hipMemcpy(out_raw, run.d_out, run.out_bytes, hipMemcpyDeviceToHost));
    if (run.pooled) HIP_TRY(hipMemcpy(pool_raw, run.d_pool, run.pool_bytes, hipMemcpyDeviceToHost));
    return MI_UNET_OK;
}

int mi_unet_debug_layer_count(const mi_unet_t *h) { return h ? (int)h->plan.size() : 0; }

int mi_unet_debug_layer_info(const mi_unet_t *h, int layer, mi_unet_layer_info *info)
{
    if (!h || !info) return fail(MI_UNET_EARG, "mi_unet_debug_layer_info: null argument");
    if (!h->weights_loaded) return fail(MI_UNET_ESTATE, "Engine not initialized: load weights before inference");
    if (layer < 0 || layer >= (int)h->plan.size()) return fail(MI_UNET_EARG, "mi_unet_debug_layer_info: no such layer");
    const Step &st = h->plan[layer];
    *info = mi_unet_layer_info{};
    snprintf(info->name, sizeof info->name, "%s", st.name.c_str());
    switch (st.kind) {
    case Step::FIRST: info->kind = 0; info->in_h = info->out_h = st.H; info->in_w = info->out_w = st.W; info->in_c = st.C; info->out_c = st.Cout; break;
    case Step::CONV: info->kind = 1; info->in_h = info->out_h = st.a.H; info->in_w = info->out_w = st.a.W; info->in_c = st.a.Cin; info->out_c = st.a.Cout; break;
    case Step::CONVT: info->kind = 2; info->in_h = st.a.H; info->in_w = st.a.W; info->out_h = 2 * st.a.H; info->out_w = 2 * st.a.W; info->in_c = st.a.Cin; info->out_c = st.a.Cout; break;
    case Step::POOL: info->kind = 3; info->in_h = st.H; info->in_w = st.W; info->out_h = st.H / 2; info->out_w = st.W / 2; info->in_c = info->out_c = st.C; break;
    case Step::HEAD: info->kind = 4; info->in_h = info->out_h = st.H; info->in_w = info->out_w = st.W; info->in_c = st.C; info->out_c = st.Cout; break;
    case Step::UPSAMPLE: info->kind = 5; info->in_h = st.H; info->in_w = st.W; info->out_h = 2 * st.H; info->out_w = 2 * st.W; info->in_c = info->out_c = st.C; break;
    }
    return MI_UNET_OK;
}

int mi_unet_debug_capture(mi_unet_t *h, const uint8_t *imgs, int B, int layer, int img, float *in, float *out, float *pooled,
                          uint8_t *labels, mi_unet_layer_info *info)
{
    if (int rc = check_handle(h, true)) return rc;
    if (!imgs || !info || B < 1 || B > h->cfg.max_batch || img < 0 || img >= B)
        return fail(MI_UNET_EARG, "mi_unet_debug_capture: bad argument (1 <= B <= max_batch, 0 <= img < B)");
    if (int rc = mi_unet_debug_layer_info(h, layer, info)) return rc;
    HIP_TRY(hipSetDevice(h->cfg.device));
    const size_t in_bytes = (size_t)B * h->cfg.height * h->cfg.width * h->cfg.in_ch;
    HIP_TRY(hipStreamSynchronize(h->stream));
    HIP_TRY(hipMemcpy(h->d_img, imgs, in_bytes, hipMemcpyHostToDevice));
    h->tap = mi_unet::Tap{};
    h->tap.layer = layer; h->tap.img = img; h->tap.in = in; h->tap.out = out; h->tap.pooled = pooled; h->tap.labels = labels; h->tap.info = info;
    const int rc = launch_plan(h, h->d_img, B, h->d_labels, h->d_logits);       // eager: the kernels a batch of B takes
    const bool hit = h->tap.hit;
    h->tap = mi_unet::Tap{};
    const hipError_t es = hipStreamSynchronize(h->stream);
    if (rc) return rc;
    if (es != hipSuccess) return fail(MI_UNET_EHIP, std::string("hipStreamSynchronize: ") + hipGetErrorString(es));
    if (!hit) return fail(MI_UNET_ESTATE, "mi_unet_debug_capture: the plan never reached the layer");
    return MI_UNET_OK;
}

}  // extern "C"
