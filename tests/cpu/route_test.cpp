// route_test.cpp -- the kernel every layer of the shipped plans is routed to (csrc/routing.cpp), on a CPU.  The plan is the engine's
// own: engine_pack_weights (csrc/weights.cpp) lays out a real weight file, build_plan and route_plan (csrc/plan.cpp) run on made-up
// buffer addresses.  The expected names are what the engine launched before the routing had one owner: mi_unet_get_kernel_stats of
// the fp32, bf16 and fp16 plans on an MI355X (256 CUs), the same as profiles/r04_per_layer.txt, r04_bf16_per_layer.txt and
// r04_fp16_per_layer.txt where those cover the case.
// Build (with real_plan.h): g++ -std=c++17 -D__HIP_PLATFORM_AMD__ -I/opt/rocm/include route_test.cpp ../../<pkg>/csrc/{routing,plan,weights}.cpp
// Run: route_test <weights of FP32> <weights of CFG5>   (MIUNETW1 files of miunet.spec, transposed decoder)
#include <map>
#include <utility>

#include "real_plan.h"

using namespace miunet;
using real_plan::dummy;
using real_plan::dummy_u8;

namespace {

struct Net { int size, in_ch, base, levels, classes, file; };    // file: index of the weight file on the command line
const Net FP32 = { 512, 1, 64, 4, 3, 0 };     // BASELINE configs 1-3 (the bf16 and fp16 plans of config 3 too)
const Net CFG5 = { 1024, 3, 32, 5, 3, 1 };    // BASELINE config 5
const char *weight_files[2];
const int MAX_BATCH = 64;

// the engine's plan of net `n` for `algo`: built once per pair
const std::vector<Step> &plan_of(const Net &n, int algo, PlanInput &in)
{
    static std::map<std::pair<int, int>, std::pair<PlanInput, std::vector<Step>>> cache;
    auto it = cache.find({ n.file, algo });
    if (it == cache.end()) {
        PlanInput pi;
        std::vector<Step> plan = real_plan::load(weight_files[n.file], n.size, n.in_ch, n.base, n.levels, n.classes, MAX_BATCH, algo, UP_TRANSPOSE, pi);
        it = cache.emplace(std::make_pair(n.file, algo), std::make_pair(pi, std::move(plan))).first;
    }
    in = it->second.first;
    return it->second.second;
}

struct Case {
    const char *what;
    Net net;
    int algo, B;
    bool guard_tripped, ksplit;
    std::vector<std::string> expect;       // per layer, in plan order
};

struct Routed { std::vector<std::string> layer, route; int convs = 0, convTs = 0; };

// The route of every conv3x3 (after the stand-alone first layer) and transposed-conv step, as route_plan launches a batch of B
// (wino4_asm = 0: a handle whose assembly kernels are switched off or did not load)
Routed route_names(const Net &n, int algo, int B, bool guard_tripped, bool ksplit, int wino4_asm = 1)
{
    PlanInput in;
    const std::vector<Step> &plan = plan_of(n, algo, in);
    in.routing.wino4_asm = wino4_asm;
    in.guard_tripped = guard_tripped;
    in.ksplit = ksplit ? dummy + 11 : nullptr;
    in.ksplit_bytes = ksplit ? (size_t)64 << 20 : 0;
    std::vector<Launch> launches;
    route_plan(in, plan, dummy_u8, B, dummy_u8, dummy + 12, real_plan::lp_kind(algo), launches);
    Routed r;
    for (size_t i = 0; i < plan.size(); ++i) {
        if (plan[i].kind != Step::CONV && plan[i].kind != Step::CONVT) continue;
        ++(plan[i].kind == Step::CONV ? r.convs : r.convTs);
        r.layer.push_back(plan[i].name);
        r.route.push_back(route_name(launches[i].rc.route, launches[i].rc.fused));
    }
    return r;
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

int main(int argc, char **argv)
{
    if (argc != 3) { printf("usage: route_test <weights of the 512 x 512 x 1 base-64 net> <weights of config 5>\n"); return 2; }
    weight_files[0] = argv[1]; weight_files[1] = argv[2];
    int bad = 0;
    for (const Case &c : cases) {
        const Routed r = route_names(c.net, c.algo, c.B, c.guard_tripped, c.ksplit);
        const std::vector<std::string> &got = r.route;
        // the plan routed is the whole network: 4 conv3x3 + 1 transposed conv per level, inc.c2 (17 + 4, config 5: 21 + 5)
        if (r.convs != 4 * c.net.levels + 1 || r.convTs != c.net.levels) { printf("%s: the plan has %d conv3x3 and %d transposed-conv steps\n", c.what, r.convs, r.convTs); ++bad; }
        if (got.size() != c.expect.size()) { printf("%s: %zu layers, expected %zu\n", c.what, got.size(), c.expect.size()); ++bad; continue; }
        for (size_t i = 0; i < got.size(); ++i)
            if (got[i] != c.expect[i]) { printf("%s: %s routed to %s, expected %s\n", c.what, r.layer[i].c_str(), got[i].c_str(), c.expect[i].c_str()); ++bad; }
    }
    // every fp32 case again as a handle without the assembly kernels routes it (Routing::wino4_asm = 0): no layer on conv3x3_wino4a /
    // conv3x3_wino4b, and every layer that was on an F(4x4,3x3) kernel still on one (the hipcc kernels conv3x3_wino4 / conv3x3_wino4s)
    for (const Case &c : cases) {
        if (c.algo != MI_UNET_CONV_WINOGRAD) continue;
        const Routed with = route_names(c.net, c.algo, c.B, c.guard_tripped, c.ksplit), r = route_names(c.net, c.algo, c.B, c.guard_tripped, c.ksplit, 0);
        if (r.route.size() != with.route.size()) { printf("%s, wino4_asm = 0: %zu layers, expected %zu\n", c.what, r.route.size(), with.route.size()); ++bad; continue; }
        for (size_t i = 0; i < r.route.size(); ++i) {
            const std::string &g = r.route[i], &w = with.route[i];
            const bool asm_kernel = g.rfind("conv3x3_wino4a", 0) == 0 || g.rfind("conv3x3_wino4b", 0) == 0;
            const bool was4 = w.rfind("conv3x3_wino4", 0) == 0, is4 = g.rfind("conv3x3_wino4", 0) == 0;
            const bool was_asm = w.rfind("conv3x3_wino4a", 0) == 0 || w.rfind("conv3x3_wino4b", 0) == 0;
            if (asm_kernel || was4 != is4 || (!was_asm && g != w)) {
                printf("%s, wino4_asm = 0: %s routed to %s (%s with the assembly kernels)\n", c.what, r.layer[i].c_str(), g.c_str(), w.c_str());
                ++bad;
            }
        }
    }
    // batch-invariant mode (MIUNET_SPLITK=0: no split-K workspace): no layer's route depends on B
    const std::vector<std::string> b1 = route_names(FP32, MI_UNET_CONV_WINOGRAD, 1, false, false).route;
    for (int B = 2; B <= 64; ++B)
        if (route_names(FP32, MI_UNET_CONV_WINOGRAD, B, false, false).route != b1) { printf("MIUNET_SPLITK=0: the routes at batch %d differ from batch 1\n", B); ++bad; }
    // the steps the engine launches itself
    if (route_name(Route::FIRST) != "conv3x3_first" || route_name(Route::POOL) != "maxpool2x2" || route_name(Route::HEAD) != "head_argmax") {
        printf("first / pool / head kernel names changed\n");
        ++bad;
    }
    // the stride bounds of the shape contracts: a pixel stride shorter than the channels it holds is refused by every one of them,
    // in either half of a concat buffer (alignment alone would let ldc = Cin - 8 or ldo = co_off + Cout - 8 through)
    {
        static const float dummy[4] = {};
        struct Row { const char *what; bool (*ok)(const ConvArgs &); int Cin, Cout, H, W, out_lp, nmul, pool; };
        const Row rows[] = {
            { "conv3x3_lpr_shape_ok", conv3x3_lpr_shape_ok, 64, 64, 16, 32, 1, 1, 1 },
            { "conv3x3_lprk_shape_ok", conv3x3_lprk_shape_ok, 128, 64, 16, 32, 1, 1, 0 },
            { "convT2x2_lpr_shape_ok", convT2x2_lpr_shape_ok, 128, 64, 16, 32, 1, 4, 0 },
            { "conv3x3_wino4a_shape_ok", conv3x3_wino4a_shape_ok, 64, 128, 16, 32, 0, 1, 1 },
            { "conv3x3_wino4b_shape_ok", conv3x3_wino4b_shape_ok, 64, 64, 16, 32, 0, 1, 1 },
        };
        for (const Row &rw : rows) {
            ConvArgs a{};
            a.in = a.wpk = a.wpk4 = a.bias = dummy;
            a.B = 1; a.H = rw.H; a.W = rw.W; a.Cin = rw.Cin; a.ldc = rw.Cin; a.Cout = rw.Cout; a.CoutPad = rw.nmul * 128;
            a.ldo = rw.Cout; a.co_off = 0; a.out_lp = rw.out_lp;
            if (rw.pool) { a.pool_out = const_cast<float *>(dummy); a.pool_ld = rw.Cout; }
            auto expect = [&](const ConvArgs &c, bool want, const char *layout) {
                if (rw.ok(c) != want) { printf("%s: %s is %s\n", rw.what, layout, want ? "refused" : "taken"); ++bad; }
            };
            expect(a, true, "the dense layout");
            ConvArgs lower = a; lower.ldo = 2 * rw.Cout;
            expect(lower, true, "the lower half");
            ConvArgs upper = lower; upper.co_off = rw.Cout;
            expect(upper, true, "the upper half");
            ConvArgs wide_in = a; wide_in.ldc = 2 * rw.Cin;
            expect(wide_in, true, "ldc = 2 * Cin");
            ConvArgs c = a; c.ldc = rw.Cin - 8;
            expect(c, false, "ldc < Cin");
            c = a; c.ldo = rw.Cout - 8;
            expect(c, false, "ldo < Cout");
            c = upper; c.ldo = 2 * rw.Cout - 8;
            expect(c, false, "ldo < co_off + Cout");
            c = a; c.co_off = -8; c.ldo = 2 * rw.Cout;
            expect(c, false, "co_off < 0");
            if (rw.pool) { c = a; c.pool_ld = rw.Cout - 8; expect(c, false, "pool_ld < Cout"); }
        }
    }
    if (bad) { printf("%d routing mismatches\n", bad); return 1; }
    printf("all routing checks passed\n");
    return 0;
}
