// routing.h -- which kernel runs a layer.  One closed list of routes, one routing function per layer kind, and every shape
// contract the routing and the launchers share.  Host code only, no HIP runtime calls (routing.cpp); the CU count and the
// MIUNET_* switches come in resolved through ConvArgs::rt.  Internal to libmiunet.so.
#pragma once
#include <string>

#include "kernels.h"

namespace miunet {

// One row per kernel entry the engine can launch: route, the kernel name the launch log reports (bench.py maps kernel families
// by these names), and the launcher call (engine.cpp expands it with the launch's `a`, the handle's assembly kernels `k` and
// stream `s`).  FIRST, POOL, HEAD and UPSAMPLE take operands of their own, not a ConvArgs: the engine launches those itself.
#define MIUNET_ROUTES(X)                                                                  \
    X(CONV_MFMA, "conv3x3_mfma", launch_conv3x3_mfma(a, s))                               \
    X(CONV_WINO, "conv3x3_wino", launch_conv3x3_wino(a, s))                               \
    X(CONV_WINO16, "conv3x3_wino16", launch_conv3x3_wino16(a, s))                         \
    X(CONV_WINO4, "conv3x3_wino4", launch_conv3x3_wino4(a, false, s))                     \
    X(CONV_WINO4_1B, "conv3x3_wino4", launch_conv3x3_wino4(a, true, s))                   \
    X(CONV_WINO4S, "conv3x3_wino4s", launch_conv3x3_wino4s(a, s))                         \
    X(CONV_WINO4A, "conv3x3_wino4a", launch_conv3x3_wino4_asm(k, AsmKernels::WINO4A, a, s)) \
    X(CONV_WINO4B, "conv3x3_wino4b", launch_conv3x3_wino4_asm(k, AsmKernels::WINO4B, a, s)) \
    X(CONV_BF16, "conv3x3_bf16", launch_conv3x3_bf16(a, s))                               \
    X(CONV_FP16, "conv3x3_fp16", launch_conv3x3_fp16(a, s))                               \
    X(CONV_BF16W, "conv3x3_bf16w", launch_conv3x3_lp2(a, false, s))                       \
    X(CONV_FP16W, "conv3x3_fp16w", launch_conv3x3_lp2(a, true, s))                        \
    X(CONV_BF16R, "conv3x3_bf16r", launch_conv3x3_lpr(a, false, s))                       \
    X(CONV_FP16R, "conv3x3_fp16r", launch_conv3x3_lpr(a, true, s))                        \
    X(CONV_BF16K, "conv3x3_bf16k", launch_conv3x3_lprk(a, false, s))                      \
    X(CONV_FP16K, "conv3x3_fp16k", launch_conv3x3_lprk(a, true, s))                       \
    X(CONVT_MFMA, "convT2x2_mfma", launch_convT2x2_mfma(a, s))                            \
    X(CONVT_TAPS, "convT2x2_taps", launch_convT2x2_taps(a, s))                            \
    X(CONVT_BF16, "convT2x2_bf16", launch_convT2x2_bf16(a, s))                            \
    X(CONVT_FP16, "convT2x2_fp16", launch_convT2x2_fp16(a, s))                            \
    X(CONVT_BF16R, "convT2x2_bf16r", launch_convT2x2_lpr(a, false, s))                    \
    X(CONVT_FP16R, "convT2x2_fp16r", launch_convT2x2_lpr(a, true, s))                     \
    X(FIRST, "conv3x3_first", hipErrorInvalidValue)                                       \
    X(POOL, "maxpool2x2", hipErrorInvalidValue)                                           \
    X(HEAD, "head_argmax", hipErrorInvalidValue)                                          \
    X(UPSAMPLE, "upsample2x_bilinear", hipErrorInvalidValue)

enum class Route {
#define MIUNET_ROUTE_ENUM(id, name, call) id,
    MIUNET_ROUTES(MIUNET_ROUTE_ENUM)
#undef MIUNET_ROUTE_ENUM
};

// Fusions a layer can be asked for: the 1x1 head + argmax in its epilogue (the last conv), the first layer in its loader (inc.c2)
enum : unsigned { FUSE_HEAD = 1, FUSE_FIRST = 2 };

// The launch log's name: the route's kernel name + "+head" / "+first" for the fusions granted
std::string route_name(Route r, unsigned fused = 0);

// What the engine knows besides the launch's arguments
struct RoutePolicy {
    int algo;                 // resolved MI_UNET_CONV_* value
    bool guard_tripped;       // the numeric guard sent every 3x3 layer to F(2x2,3x3)
    int wino4_min_wg;         // MIUNET_WINO4_MIN_WG: smallest grid F(4x4,3x3) takes without splitting K
};

struct RouteChoice {
    Route route;
    unsigned fused;           // FUSE_* bits granted
};

// conv3x3.  `a` is the launch as the engine would make it (a.B, a.rt, a.out_lp, a.ksplit_ws set; no workspace = batch-invariant
// mode, where no choice may depend on B) with the head operands filled in when FUSE_HEAD is asked for and a.first_cin = the
// image's channels when FUSE_FIRST is; the first-layer operands themselves stay null.  A fusion that is not granted is the
// caller's to undo (head operands cleared, HEAD step launched) or to skip (first-layer operands left null).
RouteChoice route_conv(const ConvArgs &a, const RoutePolicy &p, unsigned want);
Route route_convT(const ConvArgs &a, const RoutePolicy &p);
// the F(4x4,3x3) family once the layer is on it: staged (wino4s / wino4b), fused head, assembly (wino4a), two-block or one-block
Route route_wino4(const ConvArgs &a);

// ---- shape contracts: the routing asks them, and the launcher of each kernel (file named on the right) checks its arguments
// with the same predicate
bool conv3x3_wino4a_shape_ok(const ConvArgs &a);     // wino4_asm.cpp
bool conv3x3_wino4b_shape_ok(const ConvArgs &a);
bool conv3x3_wino4s_can_fuse_first(const ConvArgs &a, int first_cin);   // conv_wino4s.hip
bool conv3x3_lpr_shape_ok(const ConvArgs &a);        // conv_lpr.hip
bool conv3x3_lpr_can_fuse_first(const ConvArgs &a, int first_cin);
bool conv3x3_lprk_shape_ok(const ConvArgs &a);       // conv_lprk.hip
bool convT2x2_lpr_shape_ok(const ConvArgs &a);       // convt_lpr.hip
bool first_mfma_takes(const Routing &rt, int Cin, int Cout, int ldo, int H, int W, int out_kind);   // layers_mem.hip
// the tile shape launch_convT2x2_taps gives a layer: {MB image rows, NBK 32-channel blocks, waves per SIMD}
struct TapsShape { int mb, nbk, wps; };
TapsShape convT_taps_shape(const ConvArgs &a);

// Routing::cus from the device's CU count and the text of MIUNET_CUS (nullptr: not set).  The persistent kernels give XCD
// x = bid & 7 the slots bid >> 3 of a grid of min(tiles, cus) workgroups, so below 8 an XCD that owns tiles would have no slot and
// its tiles would never be computed: the device's count is floored at 8 (a grid of 8 on fewer CUs is an ordinary launch).
// MIUNET_CUS=<n> (tests) replaces the count by n clamped to [8, that value]: it only ever lowers the persistent grid.
int persistent_cus(int device_cus, const char *env_text);

// geometry the predicates share with the kernels (the kernel files take these values)
constexpr int LP2_TILE_ROWS = 16;                    // conv_lp2.hip LP2::TH
constexpr int LPRK_TILE_ROWS = 4, LPRK_CIN = 128, LPRK_COUT = 64;   // conv_lprk.hip LPRK
constexpr int WINO4S_FIRST_WMAX = 64;                // conv_wino4s.hip W4S::FIRST_WMAX

}  // namespace miunet
