// route_bilinear_test.cpp -- the conv3x3 layers of the bilinear decoder's plan (csrc/plan.cpp build_plan on a version 2 weight file,
// up_mode 1, laid out by csrc/weights.cpp) through route_plan and the routing of csrc/routing.cpp, on a CPU with made-up buffer
// addresses: every layer gets a route, and the shape predicate that guards the route's launcher (where routing.h has one) accepts
// the layer.  The upsample steps themselves are launched by the engine (Route::UPSAMPLE) and take no ConvArgs.  Prints the route table.
// Build: g++ -std=c++17 -D__HIP_PLATFORM_AMD__ -I/opt/rocm/include route_bilinear_test.cpp ../../<pkg>/csrc/{routing,plan,weights}.cpp
// Run: route_bilinear_test <bilinear weights of NETS[0]> <bilinear weights of NETS[1]>   (MIUNETW1 files of miunet.spec)
#include "real_plan.h"

using namespace miunet;
using real_plan::dummy;
using real_plan::dummy_u8;

namespace {

struct Net { const char *what; int size, in_ch, base, levels, classes; };
const Net NETS[] = { { "512 x 512 x 1, base 64, 4 levels", 512, 1, 64, 4, 3 }, { "1024 x 1024 x 3, base 32, 5 levels", 1024, 3, 32, 5, 3 } };

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

int main(int argc, char **argv)
{
    if (argc != 3) { printf("usage: route_bilinear_test <bilinear weights of net 0> <bilinear weights of net 1>\n"); return 2; }
    int bad = 0, checked = 0;
    for (size_t ni = 0; ni < 2; ++ni)
        for (const Plan &p : PLANS) {
            const Net &n = NETS[ni];
            const bool lp = p.algo == MI_UNET_CONV_BF16 || p.algo == MI_UNET_CONV_FP16;
            PlanInput in;
            const std::vector<Step> plan = real_plan::load(argv[1 + ni], n.size, n.in_ch, n.base, n.levels, n.classes, 16, p.algo, UP_BILINEAR, in);
            in.guard_tripped = p.guard_tripped;
            const int batches[] = { 1, 2, 4, 8, 16 };
            std::vector<std::vector<Launch>> launches(5);
            for (int b = 0; b < 5; ++b)
                route_plan(in, plan, dummy_u8, batches[b], dummy_u8, dummy + 12, real_plan::lp_kind(p.algo), launches[b]);
            printf("== %s, %s\n%-10s", n.what, p.what, "layer");
            for (int B : batches) printf(" %-22s", ("batch " + std::to_string(B)).c_str());
            printf("\n");
            // the plan routed is the whole network: 4 conv3x3 per level + inc.c2 (17, config 5: 21) and no transposed conv
            int convs = 0, convTs = 0;
            for (const Step &st : plan) { convs += st.kind == Step::CONV; convTs += st.kind == Step::CONVT; }
            if (convs != 4 * n.levels + 1 || convTs != 0) { printf("%s, %s: the plan has %d conv3x3 and %d transposed-conv steps\n", n.what, p.what, convs, convTs); ++bad; }
            for (size_t i = 0; i < plan.size(); ++i) {
                if (plan[i].kind != Step::CONV) continue;
                const char *layer = plan[i].name.c_str();
                printf("%-10s", layer);
                for (int b = 0; b < 5; ++b) {
                    const int B = batches[b];
                    const ConvArgs &a = launches[b][i].a;
                    const RouteChoice rc = launches[b][i].rc;
                    const std::string name = route_name(rc.route, rc.fused);
                    printf(" %-22s", name.c_str());
                    ++checked;
                    if (!predicate_accepts(rc.route, rc.fused, a, n.in_ch)) {
                        printf("\n%s, %s, batch %d: %s routed to %s, whose shape predicate refuses it\n", n.what, p.what, B, layer, name.c_str());
                        ++bad;
                    }
                    if (lp != (name.find("bf16") != std::string::npos || name.find("fp16") != std::string::npos)) {
                        printf("\n%s, %s, batch %d: %s routed to %s, a kernel of the other precision\n", n.what, p.what, B, layer, name.c_str());
                        ++bad;
                    }
                    if (p.guard_tripped && rc.route != Route::CONV_WINO) {
                        printf("\n%s: the tripped guard must keep %s on F(2x2,3x3)\n", n.what, layer);
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
