// route_bilinear_test.cpp -- the conv3x3 layers of the bilinear decoder's plan (engine.cpp build_plan with a version 2 weight file,
// up_mode 1) through the routing of csrc/routing.cpp, on a CPU: every layer gets a route, and the shape predicate that guards
// the route's launcher (where routing.h has one) accepts the layer.  The upsample steps themselves are launched by the engine
// (Route::UPSAMPLE) and take no ConvArgs.  Prints the route table.
// Build: g++ -std=c++17 -D__HIP_PLATFORM_AMD__ -I/opt/rocm/include route_bilinear_test.cpp ../../<pkg>/csrc/routing.cpp
#include <cstdio>
#include <string>
#include <vector>

#include "../../include/mi_unet.h"
#include "../../unet-medical-image-contour-segmentation-cpp_amd/csrc/routing.h"

using namespace miunet;

namespace {

float dummy[1];
uint8_t dummy_u8[1];

struct Net { const char *what; int size, in_ch, base, levels, classes; };
const Net NETS[] = { { "512 x 512 x 1, base 64, 4 levels", 512, 1, 64, 4, 3 }, { "1024 x 1024 x 3, base 32, 5 levels", 1024, 3, 32, 5, 3 } };

struct Layer { std::string name; ConvArgs a; };

// the conv3x3 layers of the bilinear plan, inc.c2 first (inc.c1 is the stand-alone first layer)
std::vector<Layer> bilinear_unet(const Net &n, int algo)
{
    std::vector<Layer> out;
    int ch[8];
    for (int i = 0; i <= n.levels; ++i) ch[i] = n.base << i;
    const bool packed4 = algo == MI_UNET_CONV_WINOGRAD;
    auto layer = [&](const std::string &name, int H, int cin, int cout, int ldc, int ldo, int pool_ld) {
        Layer l{ name, ConvArgs{} };
        ConvArgs &a = l.a;
        a.in = dummy; a.wpk = dummy; a.bias = dummy; a.out = dummy;
        a.wpk4 = cout % 64 == 0 && packed4 ? dummy : nullptr;
        a.H = H; a.W = H; a.Cin = cin; a.ldc = ldc; a.Cout = cout;
        a.CoutPad = (cout + NPAD - 1) / NPAD * NPAD;
        a.ldo = ldo; a.co_off = 0; a.relu = 1;
        if (pool_ld) { a.pool_out = dummy; a.pool_ld = pool_ld; }
        out.push_back(l);
    };
    const int L = n.levels;
    int H = n.size;
    layer("inc.c2", H, ch[0], ch[0], ch[0], 2 * ch[0], ch[0]);
    for (int i = 1; i <= L; ++i) {
        H /= 2;
        const std::string d = "down" + std::to_string(i);
        const int co = i == L ? ch[L - 1] : ch[i];
        layer(d + ".c1", H, ch[i - 1], co, ch[i - 1], co, 0);
        if (i < L) layer(d + ".c2", H, ch[i], ch[i], ch[i], 2 * ch[i], ch[i]);
        else layer(d + ".c2", H, co, co, co, co, 0);
    }
    for (int i = 1; i <= L; ++i) {
        const int lvl = L - i, c = ch[lvl], cout = lvl > 0 ? c / 2 : c;
        const std::string u = "up" + std::to_string(i);
        H *= 2;
        layer(u + ".c1", H, 2 * c, c, 2 * c, c, 0);
        layer(u + ".c2", H, c, cout, c, cout, 0);
    }
    return out;
}

// the predicate routing.h names for the launcher of route `r` (true where there is none)
bool predicate_accepts(Route r, unsigned fused, const ConvArgs &a, int first_cin)
{
    switch (r) {
    case Route::CONV_WINO4A: return conv3x3_wino4a_shape_ok(a);
    case Route::CONV_WINO4B: return conv3x3_wino4b_shape_ok(a);
    case Route::CONV_WINO4S: return !(fused & FUSE_FIRST) || conv3x3_wino4s_can_fuse_first(a, first_cin);
    case Route::CONV_BF16R:
    case Route::CONV_FP16R: return conv3x3_lpr_shape_ok(a) && (!(fused & FUSE_FIRST) || conv3x3_lpr_can_fuse_first(a, first_cin));
    case Route::CONV_BF16K:
    case Route::CONV_FP16K: return conv3x3_lprk_shape_ok(a);
    case Route::FIRST: case Route::POOL: case Route::HEAD: case Route::UPSAMPLE: return false;    // not conv3x3 routes
    default: return true;
    }
}

struct Plan { const char *what; int algo; bool guard_tripped; };
const Plan PLANS[] = {
    { "fp32 winograd", MI_UNET_CONV_WINOGRAD, false },
    { "fp32 winograd, guard tripped", MI_UNET_CONV_WINOGRAD, true },
    { "bf16", MI_UNET_CONV_BF16, false },
    { "fp16", MI_UNET_CONV_FP16, false },
};

}  // namespace

int main()
{
    int bad = 0, checked = 0;
    for (const Net &n : NETS)
        for (const Plan &p : PLANS) {
            const bool lp = p.algo == MI_UNET_CONV_BF16 || p.algo == MI_UNET_CONV_FP16;
            const RoutePolicy pol{ p.algo, p.guard_tripped, 256 };
            const std::vector<Layer> layers = bilinear_unet(n, p.algo);
            printf("== %s, %s\n%-10s", n.what, p.what, "layer");
            const int batches[] = { 1, 2, 4, 8, 16 };
            for (int B : batches) printf(" %-22s", ("batch " + std::to_string(B)).c_str());
            printf("\n");
            for (size_t i = 0; i < layers.size(); ++i) {
                printf("%-10s", layers[i].name.c_str());
                for (int B : batches) {
                    ConvArgs a = layers[i].a;
                    a.B = B;
                    a.rt = Routing{};
                    a.ksplit_ws = dummy;
                    a.ksplit_ws_bytes = (size_t)64 << 20;
                    const bool last = i + 1 == layers.size();
                    a.out_lp = lp && !last;
                    unsigned want = 0;
                    if (last && (a.wpk4 != nullptr || lp)) {
                        a.head_w = dummy; a.head_b = dummy; a.head_classes = n.classes; a.head_logits = dummy; a.head_labels = dummy_u8;
                        want |= FUSE_HEAD;
                    }
                    if (i == 0) { a.first_cin = n.in_ch; want |= FUSE_FIRST; }
                    const RouteChoice rc = route_conv(a, pol, want);
                    if (!(rc.fused & FUSE_HEAD)) { a.head_w = a.head_b = nullptr; a.head_classes = 0; a.head_logits = nullptr; a.head_labels = nullptr; }
                    const std::string name = route_name(rc.route, rc.fused);
                    printf(" %-22s", name.c_str());
                    ++checked;
                    if (!predicate_accepts(rc.route, rc.fused, a, n.in_ch)) {
                        printf("\n%s, %s, batch %d: %s routed to %s, whose shape predicate refuses it\n", n.what, p.what, B, layers[i].name.c_str(), name.c_str());
                        ++bad;
                    }
                    if (lp != (name.find("bf16") != std::string::npos || name.find("fp16") != std::string::npos)) {
                        printf("\n%s, %s, batch %d: %s routed to %s, a kernel of the other precision\n", n.what, p.what, B, layers[i].name.c_str(), name.c_str());
                        ++bad;
                    }
                    if (p.guard_tripped && rc.route != Route::CONV_WINO) {
                        printf("\n%s: the tripped guard must keep %s on F(2x2,3x3)\n", n.what, layers[i].name.c_str());
                        ++bad;
                    }
                }
                printf("\n");
            }
        }
    if (route_name(Route::UPSAMPLE) != "upsample2x_bilinear") { printf("upsample kernel name changed\n"); ++bad; }
    if (bad) { printf("%d routing failures\n", bad); return 1; }
    printf("all %d bilinear routing checks passed\n", checked);
    return 0;
}
