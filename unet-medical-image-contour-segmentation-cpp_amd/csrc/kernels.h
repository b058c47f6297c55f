// kernels.h -- launch interface of the gfx950 kernels (conv_direct.hip, conv_lp.hip, conv_wino.hip, layers_mem.hip, upsample.hip, image_stages.hip, morph.hip, regions.hip, score.hip, score_volume.hip, volume.hip, tiles.hip, blend.hip).  Internal to libmiunet.so.
// The hipcc kernels are part of the library's own code object.  The two assembly kernels (csrc/asm/) are code objects of their own,
// embedded as byte blobs: an AsmKernels (below) loads them for one device when an engine is created and unloads them with the last
// handle that holds it.  libmiunet.so keeps no process-wide resource: no module, no device memory, no stream outlives its handles.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include <string>

struct mi_unet_region;      // include/mi_unet.h
struct mi_unet_score;
struct mi_unet_vcomp;
struct mi_unet_mesh_vertex;
struct mi_unet_vmeasure;
struct mi_unet_vspatial;
struct mi_unet_vmatch_side;
struct mi_unet_vmatch_pair;
struct mi_unet_vtexture;
struct mi_unet_vzones;
struct mi_unet_vzone;
struct mi_unet_vpiece;
struct mi_unet_vskel;
struct mi_unet_vbranch;
struct mi_unet_vnode;
struct mi_unet_vgraph;
struct mi_unet_vnbhood;

namespace miunet {

// Channel counts of packed weights are padded to these granules with zeros.
constexpr int KC = 16;        // input channels staged per K-chunk
constexpr int NPAD = 128;     // packed Cout granule (covers both BN = 64 and BN = 128 tiles)

// Kernel-routing switches (the MIUNET_* A/B variables) and the device's CU count, resolved ONCE per engine handle at
// mi_unet_create (once per call in mi_unet_layer_debug) and carried in every launch's arguments: a launch never calls getenv or
// touches shared tables, so cloned contexts launching from several threads share nothing mutable, and an engine's routing cannot
// change under it.  Which kernel a layer gets is decided in routing.cpp.  wino4_asm is also how the routing is TOLD that the assembly
// kernels are not there: a handle without an available() AsmKernels carries 0.
struct Routing {
    int cus = 256;            // compute units of the launch device
    int lp2 = 1;              // MIUNET_LP2: 0 never, 1 default thresholds, 2 every Cout % 128 == 0 layer
    int lpr = 1;              // MIUNET_LPR: 0 never, 1 when the tiles fill the chip four times over, 2 whatever the grid
    int lprk = 1;             // MIUNET_LPRK: the 128 -> 64 K-split resident-weight kernel (conv_lprk.hip), as lpr
    int convt_lpr = 1;        // MIUNET_CONVT_LPR: as lpr
    int wino4s = 1;           // MIUNET_WINO4S: 0 never, 1 grids that fill the chip twice over, 2 every one-block case
    int fuse_first = 1;       // MIUNET_FUSE_FIRST=0: the first layer stays a kernel of its own (A/B, parity checks)
    int wino4_asm = 1;        // MIUNET_WINO4_ASM: 0 never, 1 the hand-scheduled persistent two-block kernel for the shapes it takes
    bool convt_small = true;  // MIUNET_CONVT_SMALL=0: the per-tap transposed conv never shrinks its tile
    bool first_mfma = true;   // MIUNET_FIRST_MFMA=0: the 16-bit pipelines' first layer stays on the VALU kernel
    static Routing from_env();            // reads the environment and the current device's properties (engine.cpp)
};

// One implicit-GEMM launch: conv3x3 (taps = 9) or the 2x2-stride-2 transposed conv viewed as a 1-tap GEMM with
// N = 4*Cout (taps = 1).  Activations are NHWC fp32; `ldc`/`ldo` are the channel strides of the input / output pixel
// (so a tensor can live in one half of a concat buffer), `co_off` the first output channel written.
struct ConvArgs {
    const float *in;      // [B][H][W][ldc]
    const float *wpk;     // packed weights [nchunks][taps][CoutPad][KC]  (CoutPad counts N = 4*Cout for convT)
    const float *wpk4;    // optional second packing of the same conv3x3 for the F(4x4,3x3) kernel (see launch_conv3x3_wino4), or nullptr
    const float *bias;    // [Cout] folded BN shift (conv) or convT bias
    float *out;           // conv: [B][H][W][ldo]; convT: [B][2H][2W][ldo]
    int B, H, W;          // INPUT spatial size
    int Cin, ldc;
    int Cout;             // real output channels (convT: per-tap channels, N = 4*Cout)
    int CoutPad;          // padded N of wpk
    int ldo, co_off;
    int relu;
    // optional fused 2x2/stride-2 max pooling of the (post-ReLU) output: a second store of [B][H/2][W/2][pool_ld] at
    // channel 0.  Both conv kernels hold every 2x2 output block inside one lane, so this costs one max3 + one store.
    float *pool_out;
    int pool_ld;
    // optional split-K workspace (Winograd kernel only): when the (tile, channel) grid alone cannot fill the chip (single
    // images, deep levels) the launcher cuts K = Cin into up to 8 slices, each workgroup writes its partial 2x2 outputs into
    // slab [slice][B][H][W][Cout] and a second kernel sums the slabs in a fixed order (deterministic) and applies the
    // shift / ReLU / pooling.  nullptr or too small = never split.
    float *ksplit_ws;
    size_t ksplit_ws_bytes;
    int ksplit;           // set by the launcher
    // optional fused 1x1 head + argmax (F(4x4) one-block kernel only, Cout <= 64 so one workgroup holds every channel of
    // its pixels, no pooling): the post-ReLU tile goes through LDS instead of HBM and `out` is never written.
    //   head_w [classes][Cout], head_b [classes] (classes <= 4), planar logits [B][classes][H*W] (may be null), u8 labels
    // 16-bit kernels (conv_lp.hip): `in` always points at 16-bit activations (bf16 / fp16, NHWC, ldc in elements); out_lp
    // selects a 16-bit `out` / `pool_out` (everything but the layer in front of the fp32 head)
    int out_lp;
    Routing rt;           // resolved by the caller
    const float *head_w;
    const float *head_b;
    int head_classes;
    float *head_logits;
    uint8_t *head_labels;
    // optional fused FIRST layer (conv_wino4s.hip, the fp32 plan's inc.c2): `in` is never read; the kernel builds each 16-channel
    // chunk of its 18x18 input patch from the u8 image instead -- /255 table, conv3x3 (first_cin = 1 input channel, 64 output
    // channels = this layer's Cin) + shift + ReLU, the arithmetic of conv3x3_first_kernel -- so the first layer's 1 GiB tensor is
    // neither written nor read back.  first_w is [9][1][Cin] (BN scale folded), first_shift [Cin].
    const uint8_t *first_img;
    int first_cin;                  // channels of first_img (conv_lpr.hip; conv_wino4s.hip takes one channel only)
    const float *first_lut, *first_w, *first_shift;
};

hipError_t launch_conv3x3_mfma(const ConvArgs &a, hipStream_t s);

// Winograd F(2x2,3x3) form of the same layer: a.wpk holds the TRANSFORMED weights U = G g G^T packed as
// [Cin/8][16 positions][CoutPad][8]  (WINO_KC = 8 input channels per K-chunk).  Same ConvArgs otherwise.
constexpr int WINO_KC = 8;
constexpr int WINO_SC = 32;       // input channels per raw-patch staging step (4 K-chunks: one whole 128-byte line per pixel)
hipError_t launch_conv3x3_wino(const ConvArgs &a, hipStream_t s);
// 8-wave / two-waves-per-SIMD re-tiling of the same algorithm on v_mfma_f32_16x16x4_f32; a.wpk is packed as
// [Cin/8][8 position pairs][CoutPad][16] with element 4*kq + 2*(pos & 1) + s = U_pos[k = 2*kq + s].
hipError_t launch_conv3x3_wino16(const ConvArgs &a, hipStream_t s);
// Winograd F(4x4,3x3) on v_mfma_f32_16x16x4_f32: 16 tiles (16x16 output pixels) x 128 channels per workgroup, or 64 channels
// (one_block: persistent, the only form that fuses the 1x1 head).  a.wpk4 holds U = G g G^T (6x6) packed as
// [Cin/16][36 positions][CoutPad][16]; the launcher splits K for grids that leave most CUs idle.
constexpr int WINO4_KC = 16;
constexpr int WINO4_SC = 32;
hipError_t launch_conv3x3_wino4(const ConvArgs &a, bool one_block, hipStream_t s);
// The one-block algorithm with single-buffered 70 KB of LDS and <= 256 registers, so that two workgroups share a CU
// (conv_wino4s.hip); same packing (a.wpk4), bit-identical results, no split-K; can run the first layer in its loader.
hipError_t launch_conv3x3_wino4s(const ConvArgs &a, hipStream_t s);
// The owner of the two assembly kernels' code objects on ONE device (csrc/wino4_asm.cpp).  The constructor loads both embedded code
// objects and resolves conv3x3_wino4a_f32 and conv3x3_wino4b_f32; the destructor unloads both (device set and restored, as
// DeviceWeights::~DeviceWeights does).  A handle holds it as a std::shared_ptr next to its weights: mi_unet_create makes it (fp32
// Winograd plan, MIUNET_WINO4_ASM != 0), clones share it, the last handle's mi_unet_destroy unloads.  available(): both loads and
// both look-ups succeeded on a gfx950 device; otherwise error() says why and nothing stays loaded.
class AsmKernels {
public:
    enum Which { WINO4A = 0, WINO4B = 1 };
    explicit AsmKernels(int device);
    ~AsmKernels();
    AsmKernels(const AsmKernels &) = delete;
    AsmKernels &operator=(const AsmKernels &) = delete;
    bool available() const { return error_.empty(); }
    const std::string &error() const { return error_; }
    hipFunction_t function(Which w) const { return fn_[w]; }

private:
    void unload();
    int device_;
    hipModule_t mod_[2] = {};
    hipFunction_t fn_[2] = {};
    std::string error_;
};
// WINO4A: the two-block kernel hand-scheduled in gfx950 assembly and persistent (csrc/asm/gen_wino4_asm.py): same packing (a.wpk4),
// same tensors; its contract is conv3x3_wino4a_shape_ok (routing.h).  WINO4B: its sibling for the layers with 64 output channels per
// workgroup: blocks of 16 x 32 pixels (32 tiles) x 64 channels, a wave = 32 tiles x 16 channels, V single-buffered with a transform
// phase and an MFMA phase per chunk (csrc/asm/gen_wino4b_asm.py; conv3x3_wino4b_shape_ok).  An absent or unavailable owner is an error.
hipError_t launch_conv3x3_wino4_asm(const AsmKernels *owner, AsmKernels::Which which, const ConvArgs &a, hipStream_t s);
hipError_t launch_wino_splitk_reduce(const ConvArgs &a, hipStream_t s);   // sums a.ksplit slabs of a.ksplit_ws into a.out
// Split-K, one owner for the decision (routing.cpp; tests/cpu/ksplit_test.cpp sweeps it on a CPU): the number of K slices the
// launcher of the F(4x4) kernel with nb = 1 or 2 channel blocks per wave (one-block / two-block), or of the F(2x2) kernel, gives
// this launch; 1 = the full-K kernel.  Reads a.ksplit_ws / a.ksplit_ws_bytes, the shape, the output layout and a.head_w.
int wino4_ksplit(const ConvArgs &a, int nb);
int wino_ksplit(const ConvArgs &a);
// ... and the K chunks [begin, end) slice k of ks walks: ceil(chunks / ks) chunks rounded up to whole granules, the last slice
// what is left.  granule: 1 chunk on F(4x4), WINO_SC / WINO_KC = 4 (a super-chunk of the raw patch) on F(2x2).  The two
// functions above return a ks for which no slice is empty.  Kernels and host share it.
struct KRange { int begin, end; };
constexpr KRange ksplit_range(int chunks, int ks, int k, int granule)
{
    const int per_slice = ((chunks + ks - 1) / ks + granule - 1) / granule * granule;
    const int begin = k * per_slice;
    return { begin, begin + per_slice < chunks ? begin + per_slice : chunks };
}
hipError_t launch_convT2x2_mfma(const ConvArgs &a, hipStream_t s);
// The transposed conv as four per-tap GEMMs sharing one A operand (convt_taps.hip): a.wpk4 holds the weights packed
// [ceil(Cin/32)*4 chunks of 8][4 taps (dy*2+dx)][convT_taps_cpad(Cout)][8], zero-padded; other fields as above.
inline int convT_taps_cpad(int cout) { return (cout + NPAD - 1) / NPAD * NPAD; }
hipError_t launch_convT2x2_taps(const ConvArgs &a, hipStream_t s);

// BASELINE config 3: bf16 operands, fp32 accumulate on v_mfma_f32_16x16x32_bf16 (lpr_common.h: the shape the chip clocks highest).  Activations are bf16 in HBM too (rounded
// once, RNE, by the kernel that produces them); a.wpk holds bf16 weights packed [Cin/32][taps][CoutPad][32].
constexpr int KC_BF16 = 32;
hipError_t launch_conv3x3_bf16(const ConvArgs &a, hipStream_t s);
hipError_t launch_convT2x2_bf16(const ConvArgs &a, hipStream_t s);
// the same kernels on v_mfma_f32_16x16x32_f16 (BASELINE config 5's arithmetic); a.wpk holds IEEE half weights, same packing
hipError_t launch_conv3x3_fp16(const ConvArgs &a, hipStream_t s);
hipError_t launch_convT2x2_fp16(const ConvArgs &a, hipStream_t s);
// The wide layers (Cout % 128 == 0) of the same pipelines on a 4 x 4 register tile per wave (conv_lp2.hip): half the LDS bytes
// per MFMA.  Same packing (a.wpk), same arithmetic.
hipError_t launch_conv3x3_lp2(const ConvArgs &a, bool fp16, hipStream_t s);
// The narrow layers (Cin, Cout in {32, 64}, 16-bit output, no fused head) with the weights resident in registers and a
// persistent workgroup per CU streaming input patches through an LDS ring (conv_lpr.hip).  Same packing, same arithmetic.
hipError_t launch_conv3x3_lpr(const ConvArgs &a, bool fp16, hipStream_t s);
// 128 -> 64 channels (the first convolution behind the top-level concat): the same scheme with the reduction split over a wave
// pair, partial sums through LDS (conv_lprk.hip).  Same packing; fp32 re-association differs from conv_mfma_bf16 by one add.
hipError_t launch_conv3x3_lprk(const ConvArgs &a, bool fp16, hipStream_t s);
// ... and the three largest transposed convolutions (Cin -> Cout = 64 -> 32, 128 -> 64, 256 -> 128; convt_lpr.hip)
hipError_t launch_convT2x2_lpr(const ConvArgs &a, bool fp16, hipStream_t s);

// First layer: u8 image -> (LUT /255) -> conv3x3 (Cin = 1..4) + shift + ReLU.  w is [9][Cin][Cout] (BN scale folded).
// out_kind: 0 = fp32 output, 1 = bf16, 2 = fp16 (the 16-bit pipelines keep every activation tensor 16-bit in HBM)
hipError_t launch_conv3x3_first(const uint8_t *img, const float *lut256, const float *w, const float *shift, float *out,
                                int B, int H, int W, int Cin, int Cout, int ldo, int out_kind, const Routing &rt, hipStream_t s);

hipError_t launch_maxpool2x2(const float *in, int ldc, float *out, int B, int H, int W, int C, hipStream_t s);
// the same on 16-bit post-ReLU tensors (bf16 or fp16: non-negative values order like their bit patterns)
hipError_t launch_maxpool2x2_u16(const void *in, int ldc, void *out, int B, int H, int W, int C, hipStream_t s);

// Bilinear x2 upsampling with align_corners=True (the decoder of a bilinear=True UNet, upsample.hip): in [B][H][W][ldi] ->
// channels [co_off, co_off + C) of out [B][2H][2W][ldo]; elem_kind 0 = fp32, 1 = bf16, 2 = fp16 tensors (16-bit: fp32 arithmetic,
// one RNE rounding).  Weights as PyTorch's CPU kernel computes them, in fp32.  C % 16 == 0; `in`, `out + co_off` and both pixel
// strides 16-byte aligned.
hipError_t launch_upsample2x_bilinear(const void *in, int ldi, void *out, int ldo, int co_off, int B, int H, int W, int C, int elem_kind,
                                      const Routing &rt, hipStream_t s);

// 1x1 head + first-max-wins argmax: in [npix][Cin] -> planar logits [B][classes][H*W] (may be null) + u8 labels.
hipError_t launch_head_argmax(const float *in, int Cin, const float *w, const float *bias, int classes, float *logits,
                              uint8_t *labels, int B, int HW, hipStream_t s);

// Device form of the RAW16 preprocessing arithmetic (reference: src/preprocess.cpp:65-118), bit-exact:
//   minmax   : exact u16 min / max of n samples into mnmx[0], mnmx[1] (u32 words, pre-set to 65535 / 0 by the launcher)
//   resample : top-left aligned 4-tap bilinear in fp64 with the reference's operand order and NO fma contraction,
//              quantised with (uchar)(int)((v - mn) * (255.0 / (mx - mn)) + 0.5); mx = (u16)(mn + 1) when mn == mx.
hipError_t launch_minmax_u16(const uint16_t *raw, size_t n, unsigned *mnmx, hipStream_t s);
// dst_stride = bytes between consecutive output pixels (1 = planar tile; C = plane c of an interleaved HWC tile at dst + c)
hipError_t launch_resample_u8(const uint16_t *raw, int w, int h, const unsigned *mnmx, uint8_t *dst, int outW, int outH,
                              int dst_stride, hipStream_t s);

// Intensity windows (include/mi_unet.h: mi_unet_set_window).
//   window_select : the exact order statistics s[k_lo] and s[n - 1 - k_hi] of n u16 samples (k = floor(n * ppm / 1e6)) into mnmx[0],
//                   mnmx[1]: a two-pass radix select -- 256-bin histogram of the high byte, then of the low byte of the samples whose
//                   high byte holds either rank -- with per-wave histograms in LDS and one global add per non-empty bin per
//                   workgroup.  `scratch` = window_scratch_bytes() of device memory per plane, ZEROED on the stream by the caller;
//                   raw 16-byte aligned, 0 < n < 2^32 (u32 counters)
//   resample_u8_window / normalise_u16_window : launch_resample_u8 / launch_normalise_u16 with the window's quantisation: L = lo,
//                   Hh = hi > lo ? hi : lo + 1 (in int), vc = min(max(v, L), Hh), byte = (uchar)(int)((vc - L) * (255.0 / (Hh - L)) + 0.5).
//                   The pair is read from `mnmx` (window_select's slot) or, when mnmx is null, is the arguments lo, hi (a fixed window)
size_t window_scratch_bytes();
hipError_t launch_window_select_u16(const uint16_t *raw, size_t n, int clip_lo_ppm, int clip_hi_ppm, void *scratch, unsigned *mnmx,
                                    hipStream_t s);
hipError_t launch_resample_u8_window(const uint16_t *raw, int w, int h, const unsigned *mnmx, int lo, int hi, uint8_t *dst, int outW,
                                     int outH, int dst_stride, hipStream_t s);
hipError_t launch_normalise_u16_window(const uint16_t *raw, int w, int h, const unsigned *mnmx, int lo, int hi, uint8_t *dst,
                                       int dst_stride, hipStream_t s);

// Tiled inference (tiles.hip).  The grid is tile_grid.h's: tiles of th x tw with `halo`, numbered row-major.  Every
// launcher rebuilds the grid from (H, W, th, tw, halo) and checks the tile range [t0, t0 + nb) against it.
//   gather    : image u8 [H][W][C] -> tiles t0 .. t0 + nb - 1 as u8 [nb][th][tw][C].  img_bytes = bytes readable behind `img`; the
//               wide path reads the image as aligned dwords and needs img on a dword and img_bytes up to the next multiple of 4
//   normalise : u16 [h][w] + the mnmx pair of launch_minmax_u16 -> u8, the bytes of launch_resample_u8 at outW == w, outH == h;
//               dst_stride as there (1 = planar, C = plane c of an interleaved image at dst + c).  raw 16-byte aligned
//   stitch    : tile labels u8 [nb][th][tw] -> the rectangle each tile owns in labels [H][W]; tile_logits / logits (both or
//               neither) planar f32 [nb][classes][th][tw] -> [classes][H][W].  Over the tiles of a grid every pixel is written once
hipError_t launch_tile_gather(const uint8_t *img, size_t img_bytes, int H, int W, int C, int th, int tw, int halo, int t0, int nb,
                              uint8_t *tiles, hipStream_t s);
hipError_t launch_normalise_u16(const uint16_t *raw, int w, int h, const unsigned *mnmx, uint8_t *dst, int dst_stride, hipStream_t s);
hipError_t launch_tile_stitch(const uint8_t *tile_labels, const float *tile_logits, int classes, int H, int W, int th, int tw, int halo,
                              int t0, int nb, uint8_t *labels, float *logits, hipStream_t s);

// Blended tiled inference (tiles.hip, blend.hip; DESIGN.md 7.3, the definition in include/mi_unet.h).  Views k = t * nv + v,
// nv = tile_view_count(mirror), view v mirrored by tile_view_flip(mirror, v) (tile_grid.h).
//   gather_views : image u8 [H][W][C] -> views k0 .. k0 + nb - 1 as u8 [nb][th][tw][C], each cut at its tile's origin and mirrored
//   tile_blend   : their planar logits f32 [nb][classes][th][tw] -> acc [classes][H][W] += w * un-mirrored logit, per pixel in k
//                  order; w = wy[i] * wx[j] (tables of th and tw floats, mi_unet_tile_blend_weights), or 1 and only the owning
//                  tile's views when `owner`
//   blend_finalize : acc / (the weights summed in k order) -> labels u8 [H][W] (first-max-wins argmax) and logits [classes][H][W]
//                  when not null (may be acc: in place)
hipError_t launch_tile_gather_views(const uint8_t *img, size_t img_bytes, int H, int W, int C, int th, int tw, int halo, int mirror,
                                    int k0, int nb, uint8_t *tiles, hipStream_t s);
hipError_t launch_tile_blend(const float *tile_logits, int classes, int H, int W, int th, int tw, int halo, int mirror, bool owner,
                             const float *wy, const float *wx, int k0, int nb, float *acc, hipStream_t s);
hipError_t launch_blend_finalize(const float *acc, int classes, int H, int W, int th, int tw, int halo, int mirror, bool owner,
                                 const float *wy, const float *wx, uint8_t *labels, float *logits, hipStream_t s);

// Device form of postprocess_mask (reference: src/postprocess.cpp:13-79), integer-exact, for K targets at once (include/mi_unet.h:
// mi_unet_set_targets); the reference's own chain is the table { 1, { 2 }, { min_area } }.  One label map u8 [B][H][W], read in
// place, never replicated; out u8 [B][K][H][W].  Plane p = b * K + k is the chain on image p / K with `== cls[p % K]` and
// min_area[p % K], its output in {0, cls[p % K]}:
//   hole fill : 8-connected components of (label != cls) by lock-free union-find, per-root area + bbox by atomics; a
//               component is filled iff its bbox touches no image edge and area < min_area
//   close     : dilate then erode by the target's element of radius close_r (include/mi_unet.h: mi_unet_set_morph; off at 0)
//   open      : erode then dilate by its element of radius open_r, windows clipped to the image; the reference's is the 3x3 box
//   filter    : 8-connected components of the opened mask, kept iff area >= min_area
// Every kernel runs over the B * K planes: the number of launches does not depend on K.  The table travels as a kernel argument (at
// most POSTPROCESS_MAX_TARGETS entries).  Workspace: postprocess_workspace_bytes(B * K, H, W); B * K * H * W must not exceed
// 2^31 - 1.  With K == 1 `out` may be `labels` (in place: the last kernel, the only one that writes `out`, reads no labels and runs
// behind every kernel that does); with K > 1 an `out` that overlaps the label maps is refused with hipErrorInvalidValue.
size_t postprocess_workspace_bytes(int B, int H, int W);
constexpr int POSTPROCESS_MAX_TARGETS = 5;
constexpr int POSTPROCESS_MORPH_MAX_R = 31;             // = MI_UNET_MORPH_MAX_R
struct TargetTable {
    int K = 0;
    int cls[POSTPROCESS_MAX_TARGETS] = {};
    int min_area[POSTPROCESS_MAX_TARGETS] = {};
    // the element of the target's close / open (mi_unet_morph): the default is the reference's 3x3 open, { RECT, 1, 0 }
    int shape[POSTPROCESS_MAX_TARGETS] = {};
    int open_r[POSTPROCESS_MAX_TARGETS] = { 1, 1, 1, 1, 1 };
    int close_r[POSTPROCESS_MAX_TARGETS] = {};
};
hipError_t launch_postprocess_masks_multi(const uint8_t *labels, uint8_t *out, int B, int H, int W, const TargetTable &t, void *ws,
                                          hipStream_t s);
// The close and open of the chain for tables other than the default (morph.hip): `planes` binary planes u8 [H][W] in
// `a` (0 / non-zero; plane p is target p % t.K) -> 0 / 255 planes in *result, which is `a` or `b` (same size; both are written).  One
// launch per erosion or dilation over all planes, each plane with its own shape and radius; a step whose radius is 0 for every
// target is not launched.  Radii within 0 .. POSTPROCESS_MORPH_MAX_R.
bool morph_is_default(const TargetTable &t);            // every target { RECT, 1, 0 }: the 3x3 kernels of image_stages.hip serve it
hipError_t launch_morph_chain(uint8_t *a, uint8_t *b, int planes, int H, int W, const TargetTable &t, uint8_t **result, hipStream_t s);

// Device form of Mask2Polygon::extract_contours (reference: src/mask2polygon.cpp:29-36 = threshold 127 +
// findContours(RETR_EXTERNAL, CHAIN_APPROX_SIMPLE)), exact point sequences and contour order.
//   masks u8 [B][H][W] (any values; > 127 = foreground).  Per image: at most cap_contours contours and cap_points points.
//   out_xy     int32 [B][cap_points][2]   points of all contours of the image, contour after contour (newest first)
//   out_start  int32 [B][cap_contours+1]  first point of contour c; entry n_contours = total points
//   out_count  int32 [B]                  number of contours, or -1 when a capacity was too small
// Workspace: contour_workspace_bytes(B, H, W, cap_contours).
// mask_to_image (src/process.cpp:178-185) behind postprocess_mask: a target's mask holds {0, cls}, its picture 0 / 255 (in place
// allowed).  For cls == 2 these are the reference's bytes; its 1 -> 128 never meets a postprocessed mask.
hipError_t launch_mask_to_image_binary(const uint8_t *masks, uint8_t *vis, size_t n, hipStream_t s);
size_t contour_workspace_bytes(int B, int H, int W, int cap_contours);
hipError_t launch_extract_contours(const uint8_t *masks, int B, int H, int W, int *out_xy, int cap_points, int *out_start,
                                   int cap_contours, int *out_count, void *ws, hipStream_t s);

// The two halves of launch_extract_contours on one workspace: labelling (threshold, both forests, the sorted external roots and their
// number per plane) and the trace.  The labelling half alone serves the region measurement below.
hipError_t launch_label_contours(const uint8_t *masks, int B, int H, int W, int cap_contours, void *ws, hipStream_t s);
hipError_t launch_trace_contours(int B, int H, int W, int *out_xy, int cap_points, int *out_start, int cap_contours, int *out_count,
                                 void *ws, hipStream_t s);

// Region measurement (regions.hip; include/mi_unet.h: mi_unet_set_measure), behind launch_label_contours on the same
// workspace (the trace may run before, between or after: neither touches what the other reads or writes).
//   planes masks of H x W were labelled; plane p belongs to image p / K.  tiles u8 [planes / K][H][W][in_ch] or null, `channel` of
//   it is measured.  regions [planes][cap_contours] out: entry c describes contour c of the plane; zero behind the plane's count and
//   for a plane with more than cap_contours external components.  rcounts [planes] out: that number, or -1.  No workspace of its own.
hipError_t launch_measure_regions(int planes, int H, int W, int K, const uint8_t *tiles, int in_ch, int channel,
                                  ::mi_unet_region *regions, int *rcounts, int cap_contours, void *ws, hipStream_t s);

// Scores against ground truth (score.hip; include/mi_unet.h: mi_unet_score_labels).  pred, truth u8 [B][H][W] on the
// device; plane b * n + k compares { pred == v[k] } with { truth == v[k] } of image b.  One launch sequence for all B * n planes:
//   counts  : tp / fp / fn of every value and, with classes > 0, the confusion matrix -- both maps read once
//   columns : per plane and set, the boundary and the uncapped vertical distance g to the nearest boundary pixel of the column
//   rows    : at the source boundary pixels only, d2 = min over x' of (x - x')^2 + g(x', y)^2 with the whole row of g in LDS;
//             maximum, sum of d2, sum of floor(2^16 sqrt(d2)), and the values themselves into the direction's list
//   select  : the order statistic n - 1 - floor(n * ppm / 1e6) of either direction and of both together, 16 + 16-bit radix select
// scores [B * n] out (device).  With classes > 0, *conf receives where the u64 [B][classes][classes] matrix and behind it the [B]
// skipped counts lie inside the workspace.  Workspace: score_workspace_bytes(B, H, W, n, classes), not zeroed by the caller.
// H, W in 1 .. 32767, B * n * H * W < 2^31.
constexpr int SCORE_MAX_VALUES = 8;                     // = MI_UNET_SCORE_MAX_VALUES
struct ScoreValues { int n = 0; int v[SCORE_MAX_VALUES] = {}; };
size_t score_workspace_bytes(int B, int H, int W, int n, int classes);
hipError_t launch_score(const uint8_t *pred, const uint8_t *truth, int B, int H, int W, const ScoreValues &vals, int quantile_ppm,
                        int classes, void *ws, ::mi_unet_score *scores, const unsigned long long **conf, hipStream_t s);

// Scores of a stack as one volume (score_volume.hip; include/mi_unet.h: mi_unet_score_volume).  pred, truth u8
// [D][H][W] on the device; plane k compares { pred == v[k] } with { truth == v[k] } over the whole volume.  One launch sequence for
// all n planes:
//   counts  : score.hip's, over D * H * W voxels as one image
//   columns : per plane and set, the 6-neighbour boundary, the index distance g along z to the nearest boundary voxel of the (y, x)
//             column, and a flag per (z, y) row that holds boundary voxels
//   y       : f = min over y' of (g * uz)^2 + ((y - y') * uy)^2, only in the rows the other set flagged
//   rows    : at the source boundary voxels of a flagged row, d2 = min over x' of ((x - x') * ux)^2 + f(x') with the row of f in LDS;
//             maximum, sums, and the values into the direction's list
//   select  : score.hip's radix select and final step
// scores [n] out (device).  With classes > 0, *conf receives where the u64 [classes][classes] matrix and behind it the skipped count
// lie inside the workspace.  Workspace: score_volume_workspace_bytes(D, H, W, n, classes), not zeroed by the caller.  D, H, W in
// 1 .. SCORE_VOLUME_MAX_SIDE, n * D * H * W < 2^31, units >= 1, ((W-1) ux)^2 + ((H-1) uy)^2 + ((D-1) uz)^2 < 2^31.
constexpr int SCORE_VOLUME_MAX_SIDE = 8192;             // = MI_UNET_SCORE_VOLUME_MAX_SIDE
struct ScoreVolumeArgs { int D = 0, H = 0, W = 0, ux = 1, uy = 1, uz = 1, quantile_ppm = 50000, classes = 0; ScoreValues vals; };
size_t score_volume_workspace_bytes(int D, int H, int W, int n, int classes);
hipError_t launch_score_volume(const uint8_t *pred, const uint8_t *truth, const ScoreVolumeArgs &a, void *ws, ::mi_unet_score *scores,
                               const unsigned long long **conf, hipStream_t s);

// Volume components (volume.hip; include/mi_unet.h: mi_unet_volume_components).  masks u8 [D][H][W] on the device; plane
// k is the set { masks == v[k] }.  One launch sequence for all n planes:
//   init    : run-start parents inside 64-lane segments; a run ends at x = W - 1 (so at every row, slice and plane end)
//   merge   : unions with the earlier neighbours the connectivity allows, the implied ones left out
//   roots   : every root takes a slot of its plane (a per-plane cursor) and clears the slot's statistics
//   stats   : flatten + voxels, bounding box, face counts and coordinate sums, carried per root across a wave's segments
//   keys    : the 62-bit order key of every slot; the roots that pass min_voxels are counted
//   select  : the keep_largest-th and the cap-th largest key of every plane, an exact radix select (11 bits a pass)
//   table   : the selected keys of a plane sorted by one workgroup in LDS -> table entries and the slots' table indices
//   write   : out and ids in one pass
// out u8 [n][D][H][W]; ids i32 [n][D][H][W] or null; table [n][cap]; counts i32 [2][n]: found, then kept.  Workspace:
// volume_workspace_bytes(D, H, W, n), not zeroed by the caller.  n * D * H * W < 2^31, cap <= VOLUME_MAX_TABLE.
constexpr int VOLUME_MAX_VALUES = 8;                    // = MI_UNET_VOLUME_MAX_VALUES
constexpr int VOLUME_MAX_TABLE = 4096;                  // = MI_UNET_VOLUME_MAX_TABLE
struct VolumeArgs { int D = 0, H = 0, W = 0, n = 0, cap = 0, connectivity = 26, min_voxels = 0, keep_largest = 0; int v[VOLUME_MAX_VALUES] = {}; };
size_t volume_workspace_bytes(int D, int H, int W, int n);
hipError_t launch_volume_components(const uint8_t *masks, const VolumeArgs &a, uint8_t *out, int32_t *ids, ::mi_unet_vcomp *table,
                                    int32_t *counts, void *ws, hipStream_t s);
// The exact selection of volume.hip by itself, for a stage that ranks slots of its own by the same keys (volume_split.hip): acc [n],
// key [n][S]; acc[k].nroots keys of plane k are looked at; acc[k].thr[0] = the a.keep_largest-th largest of them, thr[1] = the a.cap-th
// largest, each left alone (the caller zeroes it: every key passes) when the plane has no more keys than that.
struct VolumeRankAcc {
    unsigned nroots;                // the cursor of the plane's slots: its components
    unsigned n_min;                 // roots with voxels >= min_voxels
    unsigned overflow;              // a root found no slot (cannot happen: see slots_per_plane); the call fails instead of writing past the end
    unsigned pad;
    unsigned long long thr[2];      // the smallest key the filter's keep_largest keeps, the smallest key in the table; 0 = every key
};
size_t volume_slots_per_plane(size_t dhw);
hipError_t launch_volume_select(const VolumeArgs &a, unsigned S, VolumeRankAcc *acc, const unsigned long long *key, hipStream_t s);

// Volume clean-up (volume_clean.hip; include/mi_unet.h: mi_unet_volume_clean).  masks u8 [D][H][W] on the device; plane
// k is the set { masks == v[k] }.  One launch sequence for all n planes:
//   set / fill : the plane's set as bytes 0 / 1; with fill, volume.hip's union-find on the complement with connectivity 6, the roots
//                that reach a face flagged from the faces' own voxels, every other background voxel added
//   dilate     : three passes of a thresholded exact distance transform -- z (index distance in the column, capped at ez + 1), y (min
//                over |dy| <= ey of (g uz)^2 + (dy uy)^2, saturated at r^2 + 1), x (min over |dx| <= ex, compared with r^2)
//   erode      : the same three passes on the complement inside the volume, the result complemented
//   emit       : bytes 0 / 1 -> 0 / v[k]
// close = dilate, erode by B(close_r); open = erode, dilate by B(open_r); a ball that is the single voxel is skipped.  out u8
// [n][D][H][W]; counts u64 [n][4]: the voxels of the set at entry, behind the fill, behind the close, behind the open (a skipped step
// leaves its entry 0).  Workspace: volume_clean_workspace_bytes(D, H, W, n), not zeroed by the caller.  n * D * H * W < 2^31, units
// and radii at most VOLUME_CLEAN_MAX_R.
constexpr int VOLUME_CLEAN_MAX_R = 46340;               // = MI_UNET_VOLUME_CLEAN_MAX_R
struct VolumeCleanArgs { int D = 0, H = 0, W = 0, n = 0, ux = 1, uy = 1, uz = 1, fill = 1, close_r = 0, open_r = 0; int v[VOLUME_MAX_VALUES] = {}; };
size_t volume_clean_workspace_bytes(int D, int H, int W, int n);
hipError_t launch_volume_clean(const uint8_t *masks, const VolumeCleanArgs &a, uint8_t *out, unsigned long long *counts, void *ws,
                               hipStream_t s);
// the erosion by B(a.open_r) alone: cores u8 [n][D][H][W] = 0 / 1; counts[4 k] = the plane's voxels, counts[4 k + 3] = its core voxels
// unless the ball is the single voxel (then the cores are the set).  The same workspace.
hipError_t launch_volume_erode(const uint8_t *masks, const VolumeCleanArgs &a, uint8_t *cores, unsigned long long *counts, void *ws,
                               hipStream_t s);

// Volume split (volume_split.hip; include/mi_unet.h: mi_unet_volume_split).  masks u8 [D][H][W] on the device; plane k
// is the set { masks == v[k] }.  Exact integers: minima of unique 64-bit keys, sums, counts; nothing depends on the order of atomics.
//   launch_volume_split_seed   : the cores (launch_volume_erode), their labels by the lock-free union-find, their sizes, then the keys:
//                                a voxel of a kept core holds (0, marker), every other voxel the all-ones "unreached"; the tiles that
//                                hold a voxel of a kept core, or a neighbour of one, are flagged for round 0.
//   launch_volume_split_round  : one round of the growth: a workgroup per flagged tile of VTX_TZ x VTX_TY x VTX_TX voxels relaxes the
//                                tile in LDS to its fixed point under the halo it read, stores what changed and flags the neighbour
//                                tiles that share a changed boundary voxel for round + 1.  active[k] += the tiles of plane k that ran.
//                                The caller queues rounds until one reports no tile; rounds that find no flag do nothing.
//   launch_volume_split_finish : the rest labelled by the union-find, a slot per piece, the pieces' sums, the order (launch_volume_select),
//                                table, info and ids; res[k] = the plane's counts, found = -1 should the slot table overflow.
// Workspace: volume_split_workspace_bytes(D, H, W, n), not zeroed by the caller.  n * D * H * W < 2^31, D H W (ux + uy + uz) < 2^33.
constexpr int VSPLIT_BATCH = 8;                         // rounds queued between two looks at the activity
struct VolumeSplitArgs {
    int D = 0, H = 0, W = 0, n = 0, cap = 0, ux = 1, uy = 1, uz = 1, connectivity = 26, neck_r = 0, min_core = 1;
    int v[VOLUME_MAX_VALUES] = {};
};
struct VolumeSplitResult { long long in_voxels, core_voxels, cores, cores_kept, coreless, max_reach; int found, reserved; };
size_t volume_split_workspace_bytes(int D, int H, int W, int n);
hipError_t launch_volume_split_seed(const uint8_t *masks, const VolumeSplitArgs &a, void *ws, hipStream_t s);
hipError_t launch_volume_split_round(const uint8_t *masks, const VolumeSplitArgs &a, void *ws, int round, unsigned *active, hipStream_t s);
hipError_t launch_volume_split_finish(const uint8_t *masks, const VolumeSplitArgs &a, int32_t *ids, ::mi_unet_vcomp *table,
                                      ::mi_unet_vpiece *info, VolumeSplitResult *res, void *ws, hipStream_t s);

// Volume mesh (volume_mesh.hip; include/mi_unet.h: mi_unet_volume_mesh).  masks u8 [D][H][W] on the device; one plane,
// the set { masks == value }, per call pair.  Every output position comes from a scan: nothing depends on the order in which atomics
// arrive (the three per-axis counts are integer sums).
//   launch_volume_mesh_count: classify (one lane per voxel: its 6-bit exposure mask into the workspace, the workgroup's quad count, the
//       per-axis counts), corners (one lane per grid corner: its eight memberships -> n and o packed as the vertex's last four bytes,
//       0 = no vertex, into the corner map; the workgroup's vertex count), then the exclusive scan of both count arrays (1024 counts per
//       workgroup, the workgroups' sums scanned the same way one level up, added back) and counts u64 [5] = quads, verts, quads_x, _y, _z.
//   launch_volume_mesh_emit (after the host has read the counts): corners write their vertex at scan base + rank in the workgroup and
//       replace their map entry by that index; voxels write their quads at scan base + rank, the four indices looked up in the map.
//       Entries at keep_verts / keep_quads and beyond are dropped (the map is complete whatever keep_verts is); verts / quads may be
//       null when their keep is 0.
// Workspace: volume_mesh_workspace_bytes(D, H, W), not zeroed by the caller.  6 * (D + 1) * (H + 1) * (W + 1) < 2^31.
constexpr int VOLUME_MESH_FACES = 0, VOLUME_MESH_NETS = 1;  // = MI_UNET_MESH_FACES, _NETS
struct VolumeMeshArgs { int D = 0, H = 0, W = 0, value = 0, placement = 0; };
size_t volume_mesh_workspace_bytes(int D, int H, int W);
hipError_t launch_volume_mesh_count(const uint8_t *masks, const VolumeMeshArgs &a, unsigned long long *counts, void *ws, hipStream_t s);
hipError_t launch_volume_mesh_emit(const VolumeMeshArgs &a, void *ws, ::mi_unet_mesh_vertex *verts, int keep_verts, int32_t *quads,
                                   int keep_quads, hipStream_t s);

// Volume measurement (volume_measure.hip; include/mi_unet.h: mi_unet_volume_measure).  ids int32 [D][H][W] and intensity
// u16 [D][H][W] (or null) on the device; component r = { ids == r + 1 }, 0 <= r < m.  Every result is an integer sum, minimum or maximum:
// nothing depends on the order in which atomics arrive.  No workgroup waits for another.
//   launch_volume_measure_sums: zeroes table [m] and fills voxels, ends, the nine coordinate sums, si, sii, imax; imin holds
//       65535 - the minimum (0 = no voxel), which the caller turns round; the six diameter fields stay 0.
//   launch_volume_measure_fill (after the host has read `ends` and laid out the segments): seg[r] = (first point, points) of component r,
//       (0, 0) for one that is not searched; cursor [m] and keys [m][2] are zeroed here; every run end of a searched component goes into
//       its segment as (x ux, y uy, z uz, index), in any order.
//   launch_volume_measure_pairs: items[i] = (component, a-tile, first b-tile, b-tiles), tiles of VMS_TILE points of the component's
//       segment, a-tile <= first b-tile; a workgroup per item holds its a-tile a point per lane, takes the b-tiles through LDS and raises
//       keys[r][0] (all pairs) and keys[r][1] (pairs with equal z) to (d2 << 31) | (2^31 - 1 - the pair's smaller index).  The caller
//       bounds the pairs of one launch (volume_measure_item_pairs).
//   launch_volume_measure_ends: a workgroup per component: the smallest partner index of the winning (d2, p) of both keys ->
//       diam[r] = (d2, dp, dq, a_d2, a_p, a_q); untouched for a component that is not searched.
constexpr int VMS_TILE = 256;
struct VolumeMeasureArgs { int D = 0, H = 0, W = 0, m = 0, ux = 1, uy = 1, uz = 1; };
struct VmsItem { int comp, a_tile, b_first, b_tiles; };
hipError_t launch_volume_measure_sums(const int32_t *ids, const uint16_t *intensity, const VolumeMeasureArgs &a, ::mi_unet_vmeasure *table,
                                      hipStream_t s);
hipError_t launch_volume_measure_fill(const int32_t *ids, const VolumeMeasureArgs &a, const int2 *seg, int *cursor, unsigned long long *keys,
                                      int4 *points, hipStream_t s);
hipError_t launch_volume_measure_pairs(const int4 *points, const int2 *seg, const VmsItem *items, int n_items, unsigned long long *keys,
                                       hipStream_t s);
hipError_t launch_volume_measure_ends(const int4 *points, const int2 *seg, const unsigned long long *keys, const VolumeMeasureArgs &a,
                                      int32_t *diam, hipStream_t s);

// Volume spatial statistics (volume_spatial.hip; include/mi_unet.h: mi_unet_volume_spatial).  ids int32 [D][H][W] and
// intensity u16 [D][H][W] on the device; component r = { ids == r + 1 }, 0 <= r < m.  Integer results are sums, minima, maxima and a
// maximum under a total order: nothing depends on the order in which atomics arrive.  The pair sums are doubles: every one of them is
// added up in a fixed order, a slot per work item, no floating-point atomic.  No workgroup waits for another.
//   launch_volume_spatial_sums: zeroes table [m] and fills voxels, imax, sx, sy, sz, si, sii, six, siy, siz; imin holds 65535 - the
//       minimum (0 = no voxel), which the caller turns round; every other field stays 0.
//   launch_volume_spatial_prefix: prefix u32 [D][H][W + 1], prefix[row][k] = the sum of the row's first k intensities.
//   launch_volume_spatial_fill (after the host has read `voxels` and laid out the segments): seg[r] = (first candidate, voxels, first
//       point or -1 for a component that is not searched, centre) of component r; cursor [m] and rank [candidates] are zeroed here; every
//       voxel of a component goes into its segment, in any order, as (s << 24 | n, index, r << 1 | (v == imax)), s and n of its sphere
//       from two prefix reads per row of the ball.  rows[k] = (dy, dz, the row's x half-width, 0) of the ball's n_rows rows.
//   launch_volume_spatial_peaks: a workgroup per component: the candidate with the largest mean, ties to the smallest index, over the
//       segment and over its candidates with v == imax -> peaks[r] = (gp_sum, gp_n, gp_at, lp_sum, lp_n, lp_at); zero without a voxel.
//   launch_volume_spatial_rank: items[i] = (component, a-tile, first b-tile, b-tiles) over the whole square of the tiles of a searched
//       component's segment: rank[candidate] += the candidates of the b-tiles with a smaller index.  Integer atomics.
//   launch_volume_spatial_place: candidate -> points[first point + rank] = (x ux, y uy, z uz, v - centre): the points of a searched
//       component in index order, whatever order the fill left.
//   launch_volume_spatial_pairs: items[i] = (component, a-tile, first b-tile, b-tiles), a-tile <= first b-tile: a workgroup per item holds
//       its a-tile a point per lane, takes the b-tiles through LDS and writes slots[i] = (s0, s1, s2, s3) over the item's pairs i < j.
//       The caller bounds the pairs of one launch.
constexpr int VSP_TILE = 256;
struct VolumeSpatialArgs { int D = 0, H = 0, W = 0, m = 0, ux = 1, uy = 1, uz = 1; };
struct VspItem { int comp, a_tile, b_first, b_tiles; };
struct VspCand { unsigned long long sn; int index, tag; };     // (s << 24) | n of the voxel's sphere; its index; r << 1 | (v == imax)
hipError_t launch_volume_spatial_sums(const int32_t *ids, const uint16_t *intensity, const VolumeSpatialArgs &a, ::mi_unet_vspatial *table,
                                      hipStream_t s);
hipError_t launch_volume_spatial_prefix(const uint16_t *intensity, const VolumeSpatialArgs &a, uint32_t *prefix, hipStream_t s);
hipError_t launch_volume_spatial_fill(const int32_t *ids, const uint16_t *intensity, const uint32_t *prefix, const VolumeSpatialArgs &a,
                                      const ::mi_unet_vspatial *table, const int4 *seg, const int4 *rows, int n_rows, int *cursor, int *rank,
                                      size_t candidates, VspCand *cand, hipStream_t s);
hipError_t launch_volume_spatial_peaks(const VspCand *cand, const int4 *seg, int m, long long *peaks, hipStream_t s);
hipError_t launch_volume_spatial_rank(const VspCand *cand, const int4 *seg, const VspItem *items, int n_items, int *rank, hipStream_t s);
hipError_t launch_volume_spatial_place(const VspCand *cand, const int *rank, const uint16_t *intensity, const VolumeSpatialArgs &a,
                                       const int4 *seg, size_t candidates, int4 *points, hipStream_t s);
hipError_t launch_volume_spatial_pairs(const int4 *points, const int4 *seg, const VspItem *items, int n_items, double *slots, hipStream_t s);

// Volume matching (volume_match.hip; include/mi_unet.h: mi_unet_volume_match).  pred and truth int32 [D][H][W] on the
// device; a voxel's class is its id when 1 <= id <= m of its side, else 0.  table is the dense contingency table, int32 [mp + 1][mt + 1],
// row = pred class.  Every result is an integer sum or maximum: nothing depends on the order in which atomics arrive.  No workgroup waits
// for another.
//   launch_volume_match_count: zeroes table over this call's (mp + 1)(mt + 1) cells, then k_vmt_count adds every voxel whose key
//       a (mt + 1) + b is not 0 (cell [0][0] stays 0): a wave carries the counts of four keys and sends one atomic when a key is
//       displaced.
//   launch_volume_match_tables: k_vmt_rows (a wave per pred component) and k_vmt_cols (a lane per truth component walking 64 rows of the
//       table; the parts of a column meet in col_acc, mt * VMT_COL_ACC_BYTES bytes aligned to 8, zeroed here) with k_vmt_cols_end write
//       the finished side tables; k_vmt_rows also writes row_pairs [mp] = the row's partners; k_vmt_scan (one workgroup) turns them into
//       row_first [mp], the exclusive prefix, and *found; k_vmt_pairs (a wave per row) writes every pair whose position is below
//       keep_pairs at its final position, in (p, t) order.
constexpr size_t VMT_COL_ACC_BYTES = 16;
struct VolumeMatchArgs { int D = 0, H = 0, W = 0, mp = 0, mt = 0; };
hipError_t launch_volume_match_count(const int32_t *pred, const int32_t *truth, const VolumeMatchArgs &a, int32_t *table, hipStream_t s);
hipError_t launch_volume_match_tables(const int32_t *table, const VolumeMatchArgs &a, ::mi_unet_vmatch_side *pred_side,
                                      ::mi_unet_vmatch_side *truth_side, int32_t *row_pairs, int32_t *row_first, int32_t *found,
                                      void *col_acc, ::mi_unet_vmatch_pair *pairs, int keep_pairs, hipStream_t s);

// Volume texture (volume_texture.hip; include/mi_unet.h: mi_unet_volume_texture).  ids int32 [D][H][W] and intensity u16
// [D][H][W] on the device; component r = { ids == r + 1 }, 0 <= r < m.  Every result is an integer sum, minimum or maximum: nothing
// depends on the order in which atomics arrive.  No workgroup waits for another.
//   launch_volume_texture_keys: zeroes range [m] and fills it with (65535 - imin, imax) (k_vtx_range), then k_vtx_keys turns
//       ids IN PLACE into keys: (r + 1) << 8 | level for a voxel of component r, 0 for every other voxel.
//   launch_volume_texture_pairs: zeroes hist [m][L], inter [m][L][L] and axial [m][L][L] over this call's extent, then k_vtx_pairs, the
//       hot path: a workgroup takes VTX_TILES_PER_WG tiles of VTX_TZ x VTX_TY x VTX_TX voxels, each with its halo in LDS, counts its
//       voxels into hist, the pairs of the 4 offsets with dz = 0 into axial (want & VTX_WANT_AXIAL) and those of the 9 with dz = 1 into
//       inter (want & VTX_WANT_INTER).  The counts of the one component that leads a tile are kept in LDS and flushed when that
//       component changes; lds_table = false sends every count to memory (the comparison of DESIGN.md 7.15).
//   launch_volume_texture_finish: a workgroup per component: inter += axial (inter then holds the 13-offset table) when both are
//       wanted, and table[r] = (voxels = the histogram's sum, imin, imax, levels_used, sum of inter, sum of axial).
constexpr int VTX_TX = 64, VTX_TY = 8, VTX_TZ = 4, VTX_TILES_PER_WG = 8;
constexpr int VTX_WANT_AXIAL = 1, VTX_WANT_INTER = 2;
struct VolumeTextureArgs { int D = 0, H = 0, W = 0, m = 0, mode = 0, L = 32, lo = 0, width = 1; };
hipError_t launch_volume_texture_keys(int32_t *ids, const uint16_t *intensity, const VolumeTextureArgs &a, int2 *range, hipStream_t s);
hipError_t launch_volume_texture_pairs(const int32_t *keys, const VolumeTextureArgs &a, int want, bool lds_table, uint32_t *hist,
                                       uint32_t *inter, uint32_t *axial, hipStream_t s);
hipError_t launch_volume_texture_finish(const int2 *range, const VolumeTextureArgs &a, int want, const uint32_t *hist, uint32_t *inter,
                                        const uint32_t *axial, ::mi_unet_vtexture *table, hipStream_t s);

// Volume interpolation (volume_interp.hip; include/mi_unet.h: mi_unet_volume_interp).  masks u8 [D][H][W] and intensity
// u16 [D][H][W] (or null) on the device; plane v is the set { masks == v[v] } per slice.  Every result is a byte, a sample or an integer
// sum: nothing depends on the order in which atomics arrive.  No workgroup waits for another.  One launch sequence for all n planes:
//   columns : a lane per column of one slice of one plane: the index distance along y to the nearest pixel of the other state, 15 bits,
//             VINTERP_SENT = none in this column, the pixel's own state in bit 15; mixed[v][z] = 1 once a column of the slice holds both
//   rows    : the hot path.  A workgroup per row: the row of column words in LDS, a lane per pixel searches outwards and stops once
//             (ux dx)^2 reaches the best so far -> field int32 [n][D][H][W]: + e where set, - e where unset, e = VINTERP_NONE in a slice
//             that is all one state (no search there).  Computed once per slice, not once per slice pair.
//   blend   : a lane per (y, x) of the slice pair (z, z + 1) reads the two signed values once and writes the pair's k output bytes
//             (pair D - 1 is the last slice alone); counts u64 [n][D][5] = per plane and pair in_voxels, out_voxels, mixed, mixed_set,
//             ties, zeroed here, by a wave reduction, a sum in LDS and one atomic per workgroup and non-zero count; the caller adds the
//             pairs of a plane up
//   lerp    : the intensity, a lane per (y, x) of a slice pair
// out u8 [n][D'][H][W], D' = (D - 1) k + 1.  Workspace: volume_interp_workspace_bytes(D, H, W, n), not zeroed by the caller.
// n * D' * H * W < 2^31, sides at most VINTERP_MAX_SIDE, ((W - 1) ux)^2 + ((H - 1) uy)^2 < 2^31 - 1.
constexpr int VINTERP_MAX_SIDE = 8192, VINTERP_MAX_FACTOR = 16;     // = MI_UNET_SCORE_VOLUME_MAX_SIDE, MI_UNET_VINTERP_MAX_FACTOR
constexpr int VINTERP_NONE = 0x7FFFFFFF;                            // = MI_UNET_VINTERP_NONE
struct VolumeInterpArgs { int D = 0, H = 0, W = 0, n = 0, ux = 1, uy = 1, k = 1; int v[VOLUME_MAX_VALUES] = {}; };
size_t volume_interp_workspace_bytes(int D, int H, int W, int n);
hipError_t launch_volume_interp(const uint8_t *masks, const uint16_t *intensity, const VolumeInterpArgs &a, uint8_t *out,
                                uint16_t *intensity_out, unsigned long long *counts, void *ws, hipStream_t s);

// Volume zones (volume_zones.hip; include/mi_unet.h: mi_unet_volume_zones), behind launch_volume_texture_keys on its key
// stack: keys int32 [D][H][W], (r + 1) << 8 | level, 0 = no component.  Every result is an integer sum, minimum or maximum: nothing depends
// on the order in which atomics arrive.  No workgroup waits for another; every walk ends at the volume's border at the latest.
//   launch_volume_zones_part / _join: for a call whose m L^2 passes what launch_volume_texture_keys takes at once (2^22) while m L R does
//       not: part = the ids of components first .. first + count - 1 renumbered from 1, which that launcher turns into keys in place (its
//       range at range + first); join moves their component numbers back and writes them into the key stack, zeroed by the caller.
//   launch_volume_zones_runs: zeroes acc [m] and, over this call's extent, inter [m][L][R] and axial [m][L][R]; k_vzn_voxels counts
//       acc[r].voxels (a wave carries a component's count across its segments); then, with want != 0, k_vzn_runs, the hot path: 7.15's
//       tile with the halo of the backward neighbours in LDS, a lane per voxel; for each offset the lane whose backward neighbour has
//       another key starts a run and walks it forward, through LDS while inside the tile and through memory beyond it, and adds 1 to
//       cell (r, level, min(n, R) - 1) of axial (the 4 offsets with dz = 0, want & VZN_WANT_AXIAL) or of inter (the 9 with dz = 1,
//       want & VZN_WANT_INTER); the lanes of a wave that name one cell merge first.  acc[r].longest and the two clamped counts likewise.
//   launch_volume_zones_list: k_vzn_init (parent = the start of the voxel's run of one key inside its 64-lane segment), k_vzn_merge
//       (7.9's union-find, two voxels join iff their keys are equal and not 0, 26-connectivity, the implied unions left out; parents only
//       decrease, so a root is its zone's first voxel in raster order), k_vzn_sizes (size [root], a wave carries a root's count),
//       k_vzn_flags (roots per 256 voxels into scan), the exclusive scan of those counts in two levels (7.12's scheme: no look-back,
//       nobody waits) with *found, k_vzn_list: the records whose position is below keep_zones at their final position, `first`
//       ascending, and k_vzn_tally: acc[r].zones and acc[r].largest from every root, a wave carrying a component's count.  scan holds vzn_scan_ints(D * H * W) ints.
//   launch_volume_zones_finish: a workgroup per component: inter += axial (inter then holds the 13-offset table) when both are wanted,
//       and table[r] from range[r], acc[r] and the tables' sums.
constexpr int VZN_WANT_AXIAL = 1, VZN_WANT_INTER = 2;
constexpr size_t kVznEagerZones = 65536;                // records that travel with the first copy (volume_zones.cpp)
struct VolumeZonesArgs { int D = 0, H = 0, W = 0, m = 0, L = 32, R = 32; };
struct VznAcc { int voxels, longest, zones, largest; unsigned long long clamped_axial, clamped_inter; };      // 32 bytes
size_t vzn_scan_ints(size_t dhw);
hipError_t launch_volume_zones_part(const int32_t *ids, const VolumeZonesArgs &a, int first, int count, int32_t *part, hipStream_t s);
hipError_t launch_volume_zones_join(const int32_t *part, const VolumeZonesArgs &a, int first, int32_t *keys, hipStream_t s);
hipError_t launch_volume_zones_runs(const int32_t *keys, const VolumeZonesArgs &a, int want, VznAcc *acc, uint32_t *inter, uint32_t *axial,
                                    hipStream_t s);
hipError_t launch_volume_zones_list(const int32_t *keys, const VolumeZonesArgs &a, int32_t *parent, int32_t *size, int32_t *scan, VznAcc *acc,
                                    ::mi_unet_vzone *zones, int keep_zones, int32_t *found, hipStream_t s);
hipError_t launch_volume_zones_finish(const int2 *range, const VolumeZonesArgs &a, int want, const VznAcc *acc, uint32_t *inter,
                                      const uint32_t *axial, ::mi_unet_vzones *table, hipStream_t s);

// Volume neighbourhoods (volume_nbhood.hip; include/mi_unet.h: mi_unet_volume_nbhood), behind launch_volume_texture_keys on
// its key stack and, for the zones, behind launch_volume_zones_list on its forest.  Every result is an integer sum, minimum or maximum:
// nothing depends on the order in which atomics arrive.  No workgroup waits for another.  Tables are cleared over this call's extent.
//   launch_volume_nbhood_gather: clears the tables named in `want`, then k_vnb_gather, the hot path: 7.15's tile with its full halo
//       (6 x 10 x 66 keys) in LDS, a lane per voxel reads its 26 neighbours there and forms c, S and k over N26 and over N8 in one
//       sweep; per wanted table one count and one diff.  With lds_table the counts of the component that leads a tile are kept in
//       workgroup-private LDS tables (the diff in 32 bits there) and flushed when the leader changes; without it every count goes to
//       memory after a wave merge (k_vzn_runs' scheme).  kVnbLdsTable is what mi_unet_volume_nbhood passes (DESIGN.md 7.18 has both timings).
//   launch_volume_nbhood_dist: the multi-label L1 distance transform, separable: k_vnb_dist_x (a wave per row, segmented scans forward
//       and backward in chunks of 64), k_vnb_dist_y and k_vnb_dist_z (a lane per column, coalesced along x).  axial [D][H][W] u16 holds
//       d_axial after y; full (or NULL: no z pass) holds d.
//   launch_volume_nbhood_zones: the minimum of d and of d_axial per root of the forest (zmin, zmin_axial: int [D][H][W], a wave merges
//       before the atomic), the component's deepest, then from every root one count into dzm / dzm_axial and the clamped counts.
//   launch_volume_nbhood_finish: a workgroup per component writes the entry from range, zacc (voxels, zones), acc and the tables' sums.
constexpr int VNB_WANT_NGT = 1, VNB_WANT_DEP = 2, VNB_WANT_NGT_AXIAL = 4, VNB_WANT_DEP_AXIAL = 8, VNB_WANT_DZM = 16, VNB_WANT_DZM_AXIAL = 32;
constexpr int VNB_COLS = 27, VNB_COLS_AXIAL = 9;
constexpr bool kVnbLdsTable = true;
struct VolumeNbhoodArgs { int D = 0, H = 0, W = 0, m = 0, L = 32, alpha = 0, Dm = 32; };
struct VnbAcc { int deepest, deepest_axial; uint32_t clamped, clamped_axial; };                 // 16 bytes
struct VnbTables { uint32_t *count, *dep, *count_axial, *dep_axial, *dzm, *dzm_axial; unsigned long long *diff, *diff_axial; };
hipError_t launch_volume_nbhood_gather(const int32_t *keys, const VolumeNbhoodArgs &a, int want, bool lds_table, const VnbTables &t, hipStream_t s);
hipError_t launch_volume_nbhood_dist(const int32_t *keys, const VolumeNbhoodArgs &a, uint16_t *axial, uint16_t *full, hipStream_t s);
hipError_t launch_volume_nbhood_zones(const int32_t *keys, const VolumeNbhoodArgs &a, int want, const int32_t *parent, const uint16_t *axial,
                                      const uint16_t *full, int32_t *zmin, int32_t *zmin_axial, VnbAcc *acc, const VnbTables &t, hipStream_t s);
hipError_t launch_volume_nbhood_finish(const int2 *range, const VolumeNbhoodArgs &a, int want, const VznAcc *zacc, const VnbAcc *acc,
                                       const VnbTables &t, ::mi_unet_vnbhood *table, hipStream_t s);

// Volume skeleton (volume_skeleton.hip; include/mi_unet.h: mi_unet_volume_skeleton).  cur i32 [D][H][W] on the device: the
// ids on entry, the state of the thinning from then on, the skeleton at the end.  Exact integers: sums, counts, minima and maxima; nothing
// depends on the order of atomics.  No workgroup waits for another and every launch has a grid fixed by (D, H, W).
//   launch_volume_skeleton_begin  : ids outside 1 .. m become 0, voxels_in counted, the table cleared; with want_dist the exact squared
//                                   distance to the nearest voxel of another id, the volume wrapped in one layer of "nothing": z (a lane
//                                   per column), y and x (a lane per voxel, the scan cut off where the step alone reaches the best so far).
//   launch_volume_skeleton_pass   : one pass of the schedule: the pass state cleared, the end points marked (7.15's tile with its halo in
//                                   LDS), then per phase the candidates compacted into eight lists, one per subfield, and eight sub-step
//                                   launches, each over its list.  pass_state->deleted = what the pass deleted.
//   launch_volume_skeleton_finish : one sweep over the skeleton in the same tile: neighbour counts, link classes and radii per component
//                                   (a wave merges per id before its atomics), r2 [D][H][W] written when not null, the table finished.
//   launch_volume_skeleton_simple : the kernels' simple-point test on codes 32 first_word .. 32 (first_word + n_words) - 1 as bits.
// Workspace: volume_skeleton_workspace_bytes(D, H, W), not zeroed by the caller.  D H W < 2^31, m <= VOLUME_MAX_TABLE, sides at most
// SCORE_VOLUME_MAX_SIDE, ((W + 1) ux)^2 + ((H + 1) uy)^2 + ((D + 1) uz)^2 < 2^31.
struct VolumeSkeletonArgs { int D = 0, H = 0, W = 0, m = 0, ux = 1, uy = 1, uz = 1; };
struct VskPass { unsigned deleted; unsigned count[6][8]; unsigned pad[3]; };             // 208 bytes
size_t volume_skeleton_workspace_bytes(int D, int H, int W);
hipError_t launch_volume_skeleton_begin(int32_t *cur, const VolumeSkeletonArgs &a, bool want_dist, ::mi_unet_vskel *table, void *ws,
                                        hipStream_t s);
hipError_t launch_volume_skeleton_pass(int32_t *cur, const VolumeSkeletonArgs &a, void *ws, VskPass *pass_state, hipStream_t s);
hipError_t launch_volume_skeleton_finish(const int32_t *cur, const VolumeSkeletonArgs &a, bool want_dist, bool want_radius, int32_t *r2,
                                         ::mi_unet_vskel *table, void *ws, hipStream_t s);
hipError_t launch_volume_skeleton_simple(uint32_t first_word, uint32_t n_words, uint32_t *bits, hipStream_t s);

// Volume branches (volume_branches.hip; include/mi_unet.h: mi_unet_volume_branches).  cur i32 [D][H][W] on the device: the
// ids on entry, the state of the pruning from then on.  Exact integers; nothing depends on the order of atomics; no workgroup waits for
// another.  Only the classification sweep, the normalisation and the clears are proportional to the volume; the rest runs over the list
// of object voxels.
//   launch_volume_branches_begin  : ids outside 1 .. m become 0, the per-id table and `state` cleared.
//   launch_volume_branches_round  : the graph of the current state: classes (first: the sweep over key_tile.h's tile, which also makes the
//                                   list; later: degrees regathered from memory over the list), the forest of clusters and branches, each
//                                   branch's voxels and attached node voxels, the spurs flagged.  state->spurs = the spurs of that graph.
//   launch_volume_branches_delete : the flagged voxels deleted, pruned_spurs / pruned_voxels added per id.
//   launch_volume_branches_number : the nodes and the branches of the last round's graph numbered in raster order; state->found_*.
//   launch_volume_branches_rows   : rows 0 .. n_nodes - 1 and 0 .. n_branches - 1 (the host's min(found, cap)), the per-id table, the map.
// Workspace: volume_branches_workspace_bytes(D, H, W), not zeroed by the caller.  D H W < 2^31, m <= VOLUME_MAX_TABLE, sides at most
// SCORE_VOLUME_MAX_SIDE.
struct VolumeBranchesArgs { int D = 0, H = 0, W = 0, m = 0, prune_voxels = 0; };
struct VbrState { unsigned spurs, listed, found_nodes, found_branches; };                // 16 bytes
size_t volume_branches_workspace_bytes(int D, int H, int W);
hipError_t launch_volume_branches_begin(int32_t *cur, const VolumeBranchesArgs &a, ::mi_unet_vgraph *graph, VbrState *state, void *ws, hipStream_t s);
hipError_t launch_volume_branches_round(int32_t *cur, const VolumeBranchesArgs &a, bool first, VbrState *state, void *ws, hipStream_t s);
hipError_t launch_volume_branches_delete(int32_t *cur, const VolumeBranchesArgs &a, ::mi_unet_vgraph *graph, VbrState *state, void *ws, hipStream_t s);
hipError_t launch_volume_branches_number(int32_t *cur, const VolumeBranchesArgs &a, VbrState *state, void *ws, hipStream_t s);
hipError_t launch_volume_branches_rows(int32_t *cur, const int32_t *r2, const VolumeBranchesArgs &a, ::mi_unet_vnode *nodes, int n_nodes,
                                       ::mi_unet_vbranch *branches, int n_branches, ::mi_unet_vgraph *graph, int32_t *map, VbrState *state, void *ws,
                                       hipStream_t s);

}  // namespace miunet
