// route_test.cpp -- the kernel every layer of the shipped plans is routed to (csrc/routing.cpp), on a CPU.  The expected names are
// what the engine launched before the routing had one owner: mi_unet_get_kernel_stats of the fp32, bf16 and fp16 plans on an
// MI355X (256 CUs), the same as profiles/r04_per_layer.txt, r04_bf16_per_layer.txt and r04_fp16_per_layer.txt where those cover
// the case.  Build: g++ -std=c++17 -D__HIP_PLATFORM_AMD__ -I/opt/rocm/include route_test.cpp ../../<pkg>/csrc/routing.cpp
#include <cstdio>
#include <string>
#include <vector>

#include "../../include/mi_unet.h"
#include "../../unet-medical-image-contour-segmentation-cpp_amd/csrc/routing.h"

using namespace miunet;

namespace {

float dummy[1];
uint8_t dummy_u8[1];

struct Net { int size, in_ch, base, levels, classes; };
const Net FP32 = { 512, 1, 64, 4, 3 };        // BASELINE configs 1-3 (the bf16 and fp16 plans of config 3 too)
const Net CFG5 = { 1024, 3, 32, 5, 3 };       // BASELINE config 5

struct Layer { std::string name; bool convT; ConvArgs a; };

// The conv3x3 and transposed-conv layers of the plan (engine.cpp build_plan), inc.c2 first: input size, channels, channel
// strides of the concat buffers, fused pooling; the weights packed for F(4x4) / per-tap where the fp32 plans pack them.
std::vector<Layer> unet(const Net &n, int algo)
{
    std::vector<Layer> out;
    int ch[8];
    for (int i = 0; i <= n.levels; ++i) ch[i] = n.base << i;
    const bool packed4 = algo == MI_UNET_CONV_WINOGRAD;
    const bool lp = algo == MI_UNET_CONV_BF16 || algo == MI_UNET_CONV_FP16;
    auto layer = [&](const std::string &name, bool convT, int H, int cin, int cout, int ldo, int co_off, int pool_ld) {
        Layer l{ name, convT, ConvArgs{} };
        ConvArgs &a = l.a;
        a.in = dummy; a.wpk = dummy; a.bias = dummy; a.out = dummy;
        a.wpk4 = cout % 64 == 0 && (convT ? !lp : packed4) ? dummy : nullptr;
        a.H = H; a.W = H; a.Cin = cin; a.ldc = cin; a.Cout = cout;
        a.CoutPad = ((convT ? 4 * cout : cout) + NPAD - 1) / NPAD * NPAD;
        a.ldo = ldo; a.co_off = co_off; a.relu = !convT;
        if (pool_ld) { a.pool_out = dummy; a.pool_ld = pool_ld; }
        out.push_back(l);
    };
    int H = n.size;
    layer("inc.c2", false, H, ch[0], ch[0], 2 * ch[0], 0, ch[0]);
    for (int i = 1; i <= n.levels; ++i) {
        H /= 2;
        const std::string d = "down" + std::to_string(i);
        layer(d + ".c1", false, H, ch[i - 1], ch[i], ch[i], 0, 0);
        if (i < n.levels) layer(d + ".c2", false, H, ch[i], ch[i], 2 * ch[i], 0, ch[i]);
        else layer(d + ".c2", false, H, ch[i], ch[i], ch[i], 0, 0);
    }
    for (int i = 1; i <= n.levels; ++i) {
        const int cin = ch[n.levels - i + 1], cout = cin / 2;
        const std::string u = "up" + std::to_string(i);
        layer(u + ".t", true, H, cin, cout, 2 * cout, cout, 0);
        H *= 2;
        layer(u + ".c1", false, H, cin, cout, cout, 0, 0);
        layer(u + ".c2", false, H, cout, cout, cout, 0, 0);
    }
    return out;
}

struct Case {
    const char *what;
    Net net;
    int algo, B;
    bool guard_tripped, ksplit;
    std::vector<std::string> expect;       // per layer, in plan order
};

// The route of every layer as the engine asks for it: the last conv with the head, inc.c2 with the first layer.
std::vector<std::string> route_names(const Net &n, int algo, int B, bool guard_tripped, bool ksplit)
{
    const RoutePolicy pol{ algo, guard_tripped, 256 };
    const bool lp = algo == MI_UNET_CONV_BF16 || algo == MI_UNET_CONV_FP16;
    std::vector<Layer> layers = unet(n, algo);
    std::vector<std::string> names;
    for (size_t i = 0; i < layers.size(); ++i) {
        ConvArgs a = layers[i].a;
        a.B = B;
        a.rt = Routing{};
        if (layers[i].convT) {
            a.out_lp = lp;
            names.push_back(route_name(route_convT(a, pol)));
            continue;
        }
        const bool last = i + 1 == layers.size();
        a.ksplit_ws = ksplit ? dummy : nullptr;
        a.ksplit_ws_bytes = ksplit ? (size_t)64 << 20 : 0;
        a.out_lp = lp && !last;
        unsigned want = 0;
        if (last && (a.wpk4 != nullptr || lp)) {
            a.head_w = dummy; a.head_b = dummy; a.head_classes = n.classes; a.head_logits = dummy; a.head_labels = dummy_u8;
            want |= FUSE_HEAD;
        }
        if (i == 0) { a.first_cin = n.in_ch; want |= FUSE_FIRST; }
        const RouteChoice rc = route_conv(a, pol, want);
        names.push_back(route_name(rc.route, rc.fused));
    }
    return names;
}

const Case cases[] = {
    { "fp32, batch 16 (profiles/r04_per_layer.txt)", FP32, MI_UNET_CONV_WINOGRAD, 16, false, true, {
        "conv3x3_wino4s+first", "conv3x3_wino4a", "conv3x3_wino4a", "conv3x3_wino4a", "conv3x3_wino4a",
        "conv3x3_wino4a", "conv3x3_wino4a", "conv3x3_wino4a", "conv3x3_wino4a", "convT2x2_taps",
        "conv3x3_wino4a", "conv3x3_wino4a", "convT2x2_taps", "conv3x3_wino4a", "conv3x3_wino4a",
        "convT2x2_taps", "conv3x3_wino4a", "conv3x3_wino4a", "convT2x2_taps", "conv3x3_wino4b",
        "conv3x3_wino4s+head",
    } },
    { "fp32, batch 1: the small grids of the deep levels split K on the one-block F(4x4) kernel", FP32, MI_UNET_CONV_WINOGRAD, 1, false, true, {
        "conv3x3_wino4s+first", "conv3x3_wino4a", "conv3x3_wino4a", "conv3x3_wino4", "conv3x3_wino4",
        "conv3x3_wino4", "conv3x3_wino4", "conv3x3_wino4", "conv3x3_wino4", "convT2x2_taps",
        "conv3x3_wino4", "conv3x3_wino4", "convT2x2_taps", "conv3x3_wino4", "conv3x3_wino4",
        "convT2x2_taps", "conv3x3_wino4a", "conv3x3_wino4a", "convT2x2_taps", "conv3x3_wino4b",
        "conv3x3_wino4s+head",
    } },
    { "fp32, batch 2", FP32, MI_UNET_CONV_WINOGRAD, 2, false, true, {
        "conv3x3_wino4s+first", "conv3x3_wino4a", "conv3x3_wino4a", "conv3x3_wino4a", "conv3x3_wino4a",
        "conv3x3_wino4", "conv3x3_wino4", "conv3x3_wino4", "conv3x3_wino4", "convT2x2_taps",
        "conv3x3_wino4", "conv3x3_wino4", "convT2x2_taps", "conv3x3_wino4a", "conv3x3_wino4a",
        "convT2x2_taps", "conv3x3_wino4a", "conv3x3_wino4a", "convT2x2_taps", "conv3x3_wino4b",
        "conv3x3_wino4s+head",
    } },
    { "fp32, batch 4", FP32, MI_UNET_CONV_WINOGRAD, 4, false, true, {
        "conv3x3_wino4s+first", "conv3x3_wino4a", "conv3x3_wino4a", "conv3x3_wino4a", "conv3x3_wino4a",
        "conv3x3_wino4a", "conv3x3_wino4a", "conv3x3_wino4", "conv3x3_wino4", "convT2x2_taps",
        "conv3x3_wino4a", "conv3x3_wino4a", "convT2x2_taps", "conv3x3_wino4a", "conv3x3_wino4a",
        "convT2x2_taps", "conv3x3_wino4a", "conv3x3_wino4a", "convT2x2_taps", "conv3x3_wino4b",
        "conv3x3_wino4s+head",
    } },
    { "fp32, batch 16, numeric guard tripped: every 3x3 layer on F(2x2), first layer and head stand alone", FP32, MI_UNET_CONV_WINOGRAD, 16, true, true, {
        "conv3x3_wino", "conv3x3_wino", "conv3x3_wino", "conv3x3_wino", "conv3x3_wino",
        "conv3x3_wino", "conv3x3_wino", "conv3x3_wino", "conv3x3_wino", "convT2x2_taps",
        "conv3x3_wino", "conv3x3_wino", "convT2x2_taps", "conv3x3_wino", "conv3x3_wino",
        "convT2x2_taps", "conv3x3_wino", "conv3x3_wino", "convT2x2_taps", "conv3x3_wino",
        "conv3x3_wino",
    } },
    { "fp32, batch 1, numeric guard tripped", FP32, MI_UNET_CONV_WINOGRAD, 1, true, true, {
        "conv3x3_wino", "conv3x3_wino", "conv3x3_wino", "conv3x3_wino", "conv3x3_wino",
        "conv3x3_wino", "conv3x3_wino", "conv3x3_wino", "conv3x3_wino", "convT2x2_taps",
        "conv3x3_wino", "conv3x3_wino", "convT2x2_taps", "conv3x3_wino", "conv3x3_wino",
        "convT2x2_taps", "conv3x3_wino", "conv3x3_wino", "convT2x2_taps", "conv3x3_wino",
        "conv3x3_wino",
    } },
    { "fp32, MIUNET_SPLITK=0 (no workspace), batch 1", FP32, MI_UNET_CONV_WINOGRAD, 1, false, false, {
        "conv3x3_wino4s+first", "conv3x3_wino4a", "conv3x3_wino4a", "conv3x3_wino4a", "conv3x3_wino4a",
        "conv3x3_wino4a", "conv3x3_wino4a", "conv3x3_wino4a", "conv3x3_wino4a", "convT2x2_taps",
        "conv3x3_wino4a", "conv3x3_wino4a", "convT2x2_taps", "conv3x3_wino4a", "conv3x3_wino4a",
        "convT2x2_taps", "conv3x3_wino4a", "conv3x3_wino4a", "convT2x2_taps", "conv3x3_wino4b",
        "conv3x3_wino4s+head",
    } },
    { "bf16, batch 16 (profiles/r04_bf16_per_layer.txt)", FP32, MI_UNET_CONV_BF16, 16, false, true, {
        "conv3x3_bf16r", "conv3x3_bf16", "conv3x3_bf16w", "conv3x3_bf16w", "conv3x3_bf16w",
        "conv3x3_bf16w", "conv3x3_bf16w", "conv3x3_bf16w", "conv3x3_bf16w", "convT2x2_bf16",
        "conv3x3_bf16w", "conv3x3_bf16w", "convT2x2_bf16", "conv3x3_bf16w", "conv3x3_bf16w",
        "convT2x2_bf16r", "conv3x3_bf16w", "conv3x3_bf16w", "convT2x2_bf16r", "conv3x3_bf16k",
        "conv3x3_bf16+head",
    } },
    { "bf16, batch 1", FP32, MI_UNET_CONV_BF16, 1, false, true, {
        "conv3x3_bf16", "conv3x3_bf16", "conv3x3_bf16", "conv3x3_bf16", "conv3x3_bf16",
        "conv3x3_bf16", "conv3x3_bf16", "conv3x3_bf16", "conv3x3_bf16", "convT2x2_bf16",
        "conv3x3_bf16", "conv3x3_bf16", "convT2x2_bf16", "conv3x3_bf16", "conv3x3_bf16",
        "convT2x2_bf16", "conv3x3_bf16", "conv3x3_bf16", "convT2x2_bf16", "conv3x3_bf16k",
        "conv3x3_bf16+head",
    } },
    { "fp16, 512 x 512 x 1, batch 16", FP32, MI_UNET_CONV_FP16, 16, false, true, {
        "conv3x3_fp16r", "conv3x3_fp16", "conv3x3_fp16w", "conv3x3_fp16w", "conv3x3_fp16w",
        "conv3x3_fp16w", "conv3x3_fp16w", "conv3x3_fp16w", "conv3x3_fp16w", "convT2x2_fp16",
        "conv3x3_fp16w", "conv3x3_fp16w", "convT2x2_fp16", "conv3x3_fp16w", "conv3x3_fp16w",
        "convT2x2_fp16r", "conv3x3_fp16w", "conv3x3_fp16w", "convT2x2_fp16r", "conv3x3_fp16k",
        "conv3x3_fp16+head",
    } },
    { "fp16, BASELINE config 5 (1024 x 1024 x 3, 5 levels, base 32), batch 8 (profiles/r04_fp16_per_layer.txt)", CFG5, MI_UNET_CONV_FP16, 8, false, true, {
        "conv3x3_fp16r+first", "conv3x3_fp16r", "conv3x3_fp16r", "conv3x3_fp16", "conv3x3_fp16w",
        "conv3x3_fp16w", "conv3x3_fp16w", "conv3x3_fp16w", "conv3x3_fp16w", "conv3x3_fp16",
        "conv3x3_fp16", "convT2x2_fp16", "conv3x3_fp16w", "conv3x3_fp16w", "convT2x2_fp16",
        "conv3x3_fp16w", "conv3x3_fp16w", "convT2x2_fp16r", "conv3x3_fp16w", "conv3x3_fp16w",
        "convT2x2_fp16r", "conv3x3_fp16k", "conv3x3_fp16r", "convT2x2_fp16r", "conv3x3_fp16r",
        "conv3x3_fp16r+head",
    } },
    { "fp16, config 5, batch 1", CFG5, MI_UNET_CONV_FP16, 1, false, true, {
        "conv3x3_fp16r+first", "conv3x3_fp16", "conv3x3_fp16", "conv3x3_fp16", "conv3x3_fp16",
        "conv3x3_fp16", "conv3x3_fp16", "conv3x3_fp16", "conv3x3_fp16", "conv3x3_fp16",
        "conv3x3_fp16", "convT2x2_fp16", "conv3x3_fp16", "conv3x3_fp16", "convT2x2_fp16",
        "conv3x3_fp16", "conv3x3_fp16", "convT2x2_fp16", "conv3x3_fp16", "conv3x3_fp16",
        "convT2x2_fp16", "conv3x3_fp16k", "conv3x3_fp16", "convT2x2_fp16r", "conv3x3_fp16r",
        "conv3x3_fp16r+head",
    } },
};

}  // namespace

int main()
{
    int bad = 0;
    for (const Case &c : cases) {
        const std::vector<Layer> layers = unet(c.net, c.algo);
        const std::vector<std::string> got = route_names(c.net, c.algo, c.B, c.guard_tripped, c.ksplit);
        if (got.size() != c.expect.size()) { printf("%s: %zu layers, expected %zu\n", c.what, got.size(), c.expect.size()); ++bad; continue; }
        for (size_t i = 0; i < got.size(); ++i)
            if (got[i] != c.expect[i]) { printf("%s: %s routed to %s, expected %s\n", c.what, layers[i].name.c_str(), got[i].c_str(), c.expect[i].c_str()); ++bad; }
    }
    // batch-invariant mode (MIUNET_SPLITK=0: no split-K workspace): no layer's route depends on B
    const std::vector<std::string> b1 = route_names(FP32, MI_UNET_CONV_WINOGRAD, 1, false, false);
    for (int B = 2; B <= 64; ++B)
        if (route_names(FP32, MI_UNET_CONV_WINOGRAD, B, false, false) != b1) { printf("MIUNET_SPLITK=0: the routes at batch %d differ from batch 1\n", B); ++bad; }
    // the steps the engine launches itself
    if (route_name(Route::FIRST) != "conv3x3_first" || route_name(Route::POOL) != "maxpool2x2" || route_name(Route::HEAD) != "head_argmax") {
        printf("first / pool / head kernel names changed\n");
        ++bad;
    }
    if (bad) { printf("%d routing mismatches\n", bad); return 1; }
    printf("all routing checks passed\n");
    return 0;
}
