// routing.cpp -- which kernel runs a layer (routing.h).  Host code only: no HIP runtime calls, no environment reads in the
// product library (the MIUNET_* switches arrive resolved in ConvArgs::rt), so the same decisions can be checked on a CPU
// (tests/cpu/route_test.cpp).
#include "routing.h"

#include <cstdlib>

#include "../../include/mi_unet.h"

namespace miunet {

std::string route_name(Route r, unsigned fused)
{
    static const char *const names[] = {
#define MIUNET_ROUTE_NAME(id, name, call) name,
        MIUNET_ROUTES(MIUNET_ROUTE_NAME)
#undef MIUNET_ROUTE_NAME
    };
    std::string n = names[(int)r];
    if (fused & FUSE_HEAD) n += "+head";
    if (fused & FUSE_FIRST) n += "+first";
    return n;
}

int persistent_cus(int device_cus, const char *env_text)
{
    const int cus = device_cus < 8 ? 8 : device_cus;
    if (env_text == nullptr || *env_text == '\0') return cus;
    const int n = atoi(env_text);
    return n < 8 ? 8 : n > cus ? cus : n;
}

// ---- shape contracts

// The shapes the assembly kernel takes: whole 16x16 blocks, an even number (>= 4) of 16-channel K chunks, whole 128-channel
// groups, fp32 in and out, no fused head; every byte offset inside one image below 2^31 and the tile decode exact.
bool conv3x3_wino4a_shape_ok(const ConvArgs &a)
{
    if (a.wpk4 == nullptr || a.head_w != nullptr || a.out_lp) return false;
    if (a.B <= 0 || a.H <= 0 || a.W <= 0 || a.H % 16 || a.W % 16) return false;
    if (a.Cin % 32 || a.Cin < 64 || a.ldc % 4 || a.ldc < a.Cin) return false;
    if (a.Cout % 128 || a.CoutPad < a.Cout || a.ldo % 4 || a.co_off % 4 || a.co_off < 0 || a.ldo < a.co_off + a.Cout) return false;
    if (a.pool_out != nullptr && (a.pool_ld % 4 || a.pool_ld < a.Cout)) return false;
    const long long lim = 1ll << 31;
    if ((long long)a.H * a.W * a.ldc * 4 >= lim || (long long)a.H * a.W * a.ldo * 4 >= lim) return false;
    if ((long long)(a.Cin / 16) * 36 * a.CoutPad * 64 >= lim) return false;
    const long long m_tiles = (long long)(a.W / 16) * (a.H / 16) * a.B, nwg = m_tiles * (a.Cout / 128);
    if (nwg >= (1ll << 24) || nwg * m_tiles >= (1ll << 32)) return false;
    return true;
}

// ... and of its sibling with blocks of 16 x 32 pixels x 64 channels
bool conv3x3_wino4b_shape_ok(const ConvArgs &a)
{
    if (a.wpk4 == nullptr || a.head_w != nullptr || a.out_lp || a.first_img != nullptr) return false;
    if (a.B <= 0 || a.H <= 0 || a.W <= 0 || a.H % 16 || a.W % 32) return false;
    if (a.Cin % 32 || a.Cin < 64 || a.ldc % 4 || a.ldc < a.Cin) return false;
    if (a.Cout % 64 || a.CoutPad < a.Cout || a.ldo % 4 || a.co_off % 4 || a.co_off < 0 || a.ldo < a.co_off + a.Cout) return false;
    if (a.pool_out != nullptr && (a.pool_ld % 4 || a.pool_ld < a.Cout)) return false;
    const long long lim = 1ll << 31;
    if ((long long)a.H * a.W * a.ldc * 4 >= lim || (long long)a.H * a.W * a.ldo * 4 >= lim) return false;
    if ((long long)(a.Cin / 16) * 36 * a.CoutPad * 64 >= lim) return false;
    const long long m_tiles = (long long)(a.W / 32) * (a.H / 16) * a.B, nwg = m_tiles * (a.Cout / 64);
    if (nwg >= (1ll << 24) || nwg * m_tiles >= (1ll << 32)) return false;
    return true;
}

// the fused first layer of the staged F(4x4) kernel: one input channel, the layer's weights [9][Cin] + shift held in LDS
bool conv3x3_wino4s_can_fuse_first(const ConvArgs &a, int first_cin)
{
    return first_cin == 1 && a.Cin % WINO4_KC == 0 && a.Cin >= WINO4_KC && a.Cin <= WINO4S_FIRST_WMAX && a.head_w == nullptr && a.wpk4 != nullptr;
}

bool conv3x3_lpr_shape_ok(const ConvArgs &a)
{
    if (a.wpk == nullptr) return false;
    if (a.head_w != nullptr) {                // fused head: 32 -> 32 channels, at most three classes, fp32 tile (never stored), no pooling
        if (a.Cin != 32 || a.Cout != 32 || a.head_classes < 1 || a.head_classes > 3 || a.out_lp || a.pool_out != nullptr || a.head_labels == nullptr ||
            a.head_b == nullptr)
            return false;
    } else if (!a.out_lp) {
        return false;
    }
    if ((a.Cin != 32 && a.Cin != 64) || (a.Cout != 32 && a.Cout != 64)) return false;
    if (a.ldc % 8 || a.ldo % 8 || a.co_off % 8 || a.CoutPad < a.Cout) return false;
    if (a.ldc < a.Cin || a.co_off < 0 || a.ldo < a.co_off + a.Cout) return false;
    if (a.pool_out != nullptr && (a.pool_ld % 8 || a.pool_ld < a.Cout || (a.H & 1) || (a.W & 1))) return false;
    // 32-bit byte offsets inside one image
    return (long long)a.H * a.W * a.ldc * 2 < (1ll << 31) && (long long)a.H * a.W * a.ldo * 2 < (1ll << 31);
}

// The resident-weight kernel's fused first layer: 32 -> 32 channels behind a three-channel image (BASELINE config 5's inc.c2).
// Not 64 -> 64: see the kernel's header.
bool conv3x3_lpr_can_fuse_first(const ConvArgs &a, int first_cin)
{
    if (a.head_w != nullptr || !a.out_lp) return false;
    return first_cin == 3 && a.Cin == 32 && a.Cout == 32;
}

bool conv3x3_lprk_shape_ok(const ConvArgs &a)
{
    if (a.wpk == nullptr || !a.out_lp || a.head_w != nullptr || a.pool_out != nullptr) return false;
    if (a.Cin != LPRK_CIN || a.Cout != LPRK_COUT) return false;
    if (a.ldc % 8 || a.ldo % 8 || a.co_off % 8 || a.CoutPad < a.Cout) return false;
    if (a.ldc < a.Cin || a.co_off < 0 || a.ldo < a.co_off + a.Cout) return false;
    return (long long)a.H * a.W * a.ldc * 2 < (1ll << 31) && (long long)a.H * a.W * a.ldo * 2 < (1ll << 31);
}

// the shapes with at most 128 weight registers per wave: Cin -> Cout = 64 -> 32, 128 -> 64, 256 -> 128 (the three largest
// transposed convolutions of a base-32 or base-64 network); 16-bit output
bool convT2x2_lpr_shape_ok(const ConvArgs &a)
{
    if (a.wpk == nullptr || !a.out_lp || a.head_w != nullptr || a.pool_out != nullptr) return false;
    if (!((a.Cin == 64 && a.Cout == 32) || (a.Cin == 128 && a.Cout == 64) || (a.Cin == 256 && a.Cout == 128))) return false;
    if (a.ldc % 8 || a.ldo % 8 || a.co_off % 8 || a.CoutPad < 4 * a.Cout) return false;
    if (a.ldc < a.Cin || a.co_off < 0 || a.ldo < a.co_off + a.Cout) return false;
    return (long long)a.H * a.W * a.ldc * 2 < (1ll << 31) && 4ll * a.H * a.W * a.ldo * 2 < (1ll << 31);
}

// the MFMA form of the first layer takes the 16-bit outputs it was built for (MIUNET_FIRST_MFMA=0: never)
bool first_mfma_takes(const Routing &rt, int Cin, int Cout, int ldo, int H, int W, int out_kind)
{
    if (!rt.first_mfma) return false;
    return out_kind != 0 && (Cin == 1 || Cin == 3) && Cout % 8 == 0 && Cout <= 64 && ldo % 8 == 0 && (long long)H * W * ldo * 2 < (1ll << 31);
}

// The per-tap transposed conv's tile.  Whole batches get the measured-best shapes of DESIGN.md 4.4; when those leave the chip
// short of ~one workgroup per CU (single images, the deep levels: 32 x 32 pixels x 512 channels is 64 of the large tiles) the
// tile shrinks to one row x 128 or 64 channels with four workgroups per CU, which is latency cover for a K loop of 1024
// channels rather than operand reuse.
static long long taps_grid(const ConvArgs &a, const TapsShape &t)
{
    return (long long)((a.W + 31) / 32) * ((a.H + t.mb - 1) / t.mb) * a.B * ((a.Cout + 32 * t.nbk - 1) / (32 * t.nbk));
}
TapsShape convT_taps_shape(const ConvArgs &a)
{
#ifdef MIUNET_EXPERIMENTS                              // lab build only: the product library has one route per shape
    static const int mode = [] { const char *e = getenv("MIUNET_CONVT_WPS"); return e ? atoi(e) : 2; }();
#else
    constexpr int mode = 2;
#endif
    if (mode != 2) {
        if (a.Cout > 256) return { 1, 16, 1 };
        if (a.Cout > 128) return { 2, 8, 1 };
        if (a.Cout > 64) return { 4, 4, 1 };
        return { 8, 2, 1 };
    }
    const TapsShape big = a.Cout > 256 ? TapsShape{ 1, 8, 2 } : a.Cout > 64 ? TapsShape{ 2, 4, 2 } : TapsShape{ 4, 2, 2 };
    // MIUNET_CONVT_SMALL = 0: never shrink (parity tests of the large shapes on small inputs)
    if (taps_grid(a, big) >= 192 || !a.rt.convt_small) return big;
    if (a.Cout > 64 && taps_grid(a, { 1, 4, 4 }) >= 192) return { 1, 4, 4 };
    return { 1, 2, 4 };
}

// ---- the 16-bit kernels' takes: shape and a grid that fills the chip

// The wide layers on the 4 x 4 register tile (conv_lp2.hip).  Measured per layer at batch 16, r02: faster than the 2 x 2 kernel of
// conv_lp.hip from Cin = 256 up (down4.c2 0.280 -> 0.226 ms, up1.c1 0.552 -> 0.459), 3-5 % faster at Cin = 128 with the
// LDS-transposed stores (level with the 256-store epilogue it had first), slower below.  MIUNET_LP2: 0 = never; 2 = every
// Cout % 128 == 0 layer whatever its size (parity tests).
static bool lp2_takes(const ConvArgs &a)
{
    const int mode = a.rt.lp2;
    if (mode == 0) return false;
    if (a.head_w != nullptr || a.Cout % 128 != 0 || a.Cin % 8 || a.ldc % 8 || a.CoutPad % NPAD) return false;
    if (mode == 2) return true;
    const long long nwg = (long long)((a.W + 31) / 32) * ((a.H + LP2_TILE_ROWS - 1) / LP2_TILE_ROWS) * a.B * (a.Cout / 128);
    // from Cin = 128 since the 16-byte-store epilogue (same card, config 3: down1.c2 0.333 -> 0.322 ms, up3.c2 0.313 -> 0.298, down2.c1
    // 0.159 -> 0.154; config 5 unchanged); MIUNET_LP2_MINCIN moves the threshold
#ifdef MIUNET_EXPERIMENTS
    static const int min_cin = [] { const char *m = getenv("MIUNET_LP2_MINCIN"); return m ? atoi(m) : 128; }();
#else
    constexpr int min_cin = 128;
#endif
    return a.Cin >= min_cin && nwg >= 192;
}

// The resident-weight kernels (conv_lprk.hip 128 -> 64, conv_lpr.hip, convt_lpr.hip) when their tiles fill the chip four times
// over.  MIUNET_LPRK / MIUNET_LPR / MIUNET_CONVT_LPR = 0: never; 2: whatever the grid (parity tests on small inputs).
static bool lprk_takes(const ConvArgs &a)
{
    if (a.rt.lprk == 0 || !conv3x3_lprk_shape_ok(a)) return false;
    const long long ntiles = (long long)((a.W + 31) / 32) * ((a.H + LPRK_TILE_ROWS - 1) / LPRK_TILE_ROWS) * a.B;
    return a.rt.lprk == 2 || ntiles >= 4 * a.rt.cus;
}

static bool lpr_takes(const ConvArgs &a)
{
    if (a.rt.lpr == 0 || !conv3x3_lpr_shape_ok(a)) return false;
    const long long ntiles = (long long)((a.W + 31) / 32) * ((a.H + 15) / 16) * a.B;     // 16-row tiles (Cin = 32); twice as many of 8 rows
    return a.rt.lpr == 2 || ntiles >= 4 * a.rt.cus;
}

static bool convt_lpr_takes(const ConvArgs &a)
{
    if (a.rt.convt_lpr == 0 || !convT2x2_lpr_shape_ok(a)) return false;
    const int tr = 32 * 1024 / (a.Cin * 2) / 32;
    const long long ntiles = (long long)((a.W + 31) / 32) * ((a.H + tr - 1) / tr) * a.B;
    return a.rt.convt_lpr == 2 || ntiles >= 4 * a.rt.cus;
}

// ---- F(4x4,3x3)

// One-block cases whose grid fills the chip twice over go to the two-workgroups-per-CU kernel (conv_wino4s.hip); small grids keep
// the persistent kernel and its split-K (MIUNET_WINO4S = 0: never; 2: every one-block case whatever its grid -- parity tests on
// small shapes).
static bool wino4_staged(const ConvArgs &a)
{
    const int rem = a.Cout % 128;
    const long long wg1 = (long long)((a.W + 15) / 16) * ((a.H + 15) / 16) * a.B * ((a.Cout + 63) / 64);
    // ... and wider layers whose K loop is at most four chunks (down1.c1, 64 -> 128: 0.521 -> 0.488 ms); with eight chunks and
    // more the two-block kernel's shared forward transform wins (measured on every such layer: 7-20 % slower staged)
    // ... unless the assembly kernel can take the layer (down1.c1, 64 -> 128: 0.459 -> 0.415 ms same card, profiles/r04_ab_asm_routing.txt;
    // MIUNET_WINO4_ASM = 3 keeps such a layer on the staged kernel -- A/B switch)
    const bool asm_takes_k4 = a.rt.wino4_asm != 0 && a.rt.wino4_asm != 3 && a.Cin == 64 && conv3x3_wino4a_shape_ok(a);
    const bool one_block = a.head_w != nullptr || !(a.Cout >= 128 && (rem == 0 || rem > 64)) || (a.Cin <= 64 && !asm_takes_k4);
    // a.ksplit_ws == nullptr is the batch-invariant mode (MIUNET_SPLITK=0): there the choice must not depend on the batch
    return one_block && (a.rt.wino4s == 2 || (a.rt.wino4s == 1 && (wg1 >= 2 * a.rt.cus || a.ksplit_ws == nullptr)));
}

Route route_wino4(const ConvArgs &a)
{
    const int rem = a.Cout % 128;
    // staged layers with 64 output channels per workgroup and a shape the assembly takes: conv3x3_wino4b (rt.wino4_asm = 0: the
    // handle has no assembly kernels -- switched off, or their code objects did not load -- and neither of the two is ever chosen)
    if (wino4_staged(a)) return a.rt.wino4_asm != 0 && conv3x3_wino4b_shape_ok(a) && rem != 0 ? Route::CONV_WINO4B : Route::CONV_WINO4S;
    if (a.head_w != nullptr) return Route::CONV_WINO4_1B;
    // the hand-scheduled persistent two-block kernel takes the shapes of its contract, unless the grid is one the hipcc kernel
    // would split K for (single images, deep levels)
    const long long nwg = (long long)(a.W / 16) * (a.H / 16) * a.B * (a.Cout / 128);
    const bool split_k = a.ksplit_ws != nullptr && nwg <= 128 && a.Cin / WINO4_KC >= 8;
    if (a.rt.wino4_asm != 0 && conv3x3_wino4a_shape_ok(a) && !split_k) return Route::CONV_WINO4A;
    // 128 output channels per workgroup when Cout fills them; 64 for the Cout = 64 layers (and any Cout % 128 in (0, 64])
    return a.Cout >= 128 && (rem == 0 || rem > 64) ? Route::CONV_WINO4 : Route::CONV_WINO4_1B;
}

// ---- split-K (kernels.h): how many K slices a launch of the hipcc Winograd kernels is cut into

// the slabs [ks][B][H][W][Cout] must fit the workspace, and after rounding a slice's share up to whole granules none may be empty
static int ksplit_fit(const ConvArgs &a, int ks, int chunks, int granule)
{
    while (ks > 1 && (size_t)ks * a.B * a.H * a.W * a.Cout * sizeof(float) > a.ksplit_ws_bytes) --ks;
    while (ks > 1 && ksplit_range(chunks, ks, ks - 1, granule).begin >= chunks) --ks;
    return ks;
}

// F(4x4): split K when the (tile, channel) grid alone leaves most CUs idle; every slice keeps at least four chunks.  The reduce
// kernel moves 16 bytes at a time (Cout, ldo, co_off in fours) and knows no head.
int wino4_ksplit(const ConvArgs &a, int nb)
{
    const int nwg = ((a.W + 15) / 16) * ((a.H + 15) / 16) * a.B * ((a.Cout + 64 * nb - 1) / (64 * nb));
    const int chunks = (a.Cin + WINO4_KC - 1) / WINO4_KC;
    if (a.head_w != nullptr || a.ksplit_ws == nullptr || nwg > 128 || chunks < 8 || a.Cout % 4 || a.ldo % 4 || a.co_off % 4) return 1;
    int ks = 256 / nwg;
    if (ks > 8) ks = 8;
    if (ks > chunks / 4) ks = chunks / 4;
    return ksplit_fit(a, ks, chunks, 1);
}

// F(2x2): only when the grid cannot fill half of the 256 CUs (one workgroup per CU); each slice keeps >= 2 super-chunks
int wino_ksplit(const ConvArgs &a)
{
    const bool wide = a.Cout > 64;              // 32 tiles x 128 channels per workgroup, else 64 x 64 (launch_conv3x3_wino)
    const int tiles = ((a.W + 15) / 16) * ((a.H + (wide ? 8 : 16) - 1) / (wide ? 8 : 16)) * a.B * ((a.Cout + (wide ? 128 : 64) - 1) / (wide ? 128 : 64));
    const int chunks = (a.Cin + WINO_KC - 1) / WINO_KC;
    if (a.ksplit_ws == nullptr || tiles > 128 || chunks < 16 || a.Cout % 4 || a.ldo % 4 || a.co_off % 4) return 1;
    int ks = 256 / tiles;
    if (ks > 8) ks = 8;
    if (ks > chunks / 8) ks = chunks / 8;
    return ksplit_fit(a, ks, chunks, WINO_SC / WINO_KC);
}

// ---- the routing functions

RouteChoice route_conv(const ConvArgs &a, const RoutePolicy &p, unsigned want)
{
    const bool first = (want & FUSE_FIRST) && a.rt.fuse_first;
    if (p.algo == MI_UNET_CONV_BF16 || p.algo == MI_UNET_CONV_FP16) {
        // every 16-bit kernel that takes a layer with a head operand fuses it (the wide and the K-split kernels never take one)
        const bool fp16 = p.algo == MI_UNET_CONV_FP16;
        const unsigned head = want & FUSE_HEAD;
        if (lp2_takes(a)) return { fp16 ? Route::CONV_FP16W : Route::CONV_BF16W, head };
        if (lprk_takes(a)) return { fp16 ? Route::CONV_FP16K : Route::CONV_BF16K, head };
        if (lpr_takes(a))
            return { fp16 ? Route::CONV_FP16R : Route::CONV_BF16R, head | (first && conv3x3_lpr_can_fuse_first(a, a.first_cin) ? FUSE_FIRST : 0u) };
        return { fp16 ? Route::CONV_FP16 : Route::CONV_BF16, head };
    }
    if (p.algo == MI_UNET_CONV_WINOGRAD16) return { Route::CONV_WINO16, 0 };
    if (p.algo != MI_UNET_CONV_WINOGRAD) return { Route::CONV_MFMA, 0 };
    // F(4x4,3x3) where it was packed (Cout % 64 == 0) and its 16x16-pixel x 128-channel grid fills the chip, or the grid is so
    // small that its launcher splits K (<= 128 workgroups, >= 8 chunks of 16 channels); other small grids stay on F(2x2,3x3),
    // which can split K too.  Without a split-K workspace (MIUNET_SPLITK=0, batch-invariant mode) the choice must not depend on B.
    const long long wg4 = (long long)((a.W + 15) / 16) * ((a.H + 15) / 16) * a.B * ((a.Cout + 127) / 128);
    const bool fills = wg4 >= p.wino4_min_wg || a.ksplit_ws == nullptr;
    const bool split4 = a.ksplit_ws != nullptr && wg4 <= 128 && a.Cin >= 128 && !(want & FUSE_HEAD);
    if (a.wpk4 == nullptr || p.guard_tripped || !(fills || split4)) return { Route::CONV_WINO, 0 };
    const Route r = route_wino4(a);
    // the first layer runs in the staged kernel's loader (the assembly sibling has no such loader)
    if (first && fills && (r == Route::CONV_WINO4S || r == Route::CONV_WINO4B) && conv3x3_wino4s_can_fuse_first(a, a.first_cin))
        return { Route::CONV_WINO4S, FUSE_FIRST };
    return { r, want & FUSE_HEAD };
}

Route route_convT(const ConvArgs &a, const RoutePolicy &p)
{
    if (p.algo == MI_UNET_CONV_BF16 || p.algo == MI_UNET_CONV_FP16) {
        const bool fp16 = p.algo == MI_UNET_CONV_FP16;
        if (convt_lpr_takes(a)) return fp16 ? Route::CONVT_FP16R : Route::CONVT_BF16R;
        return fp16 ? Route::CONVT_FP16 : Route::CONVT_BF16;
    }
    // the per-tap kernel where it was packed (Cout % 64 == 0); the direct kernel below half a workgroup per CU
    return a.wpk4 != nullptr && taps_grid(a, convT_taps_shape(a)) >= 128 ? Route::CONVT_TAPS : Route::CONVT_MFMA;
}

}  // namespace miunet
