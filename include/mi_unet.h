/*
 * mi_unet.h -- C-ABI of the MI355X-native UNet segmentation engine (libmiunet.so).
 *
 * This is the drop-in seam for the reference's TensorRT call: everything between the normalised 8-bit tile and the
 * u8 label map in MedicalSeg::execute_inference (/root/reference/src/process.cpp:123-175), i.e.
 *     preprocess_image  u8 -> f32 /255.0f            src/process.cpp:22-42
 *     H2D + cudaGraphLaunch(engine) + D2H            src/process.cpp:143-155
 *     3-class first-max-wins argmax                  src/process.cpp:158-170
 * plus the lifecycle around it (engine load: src/initialize.cpp:26-77; per-thread context with device buffers, stream
 * and captured graph: src/process.cpp:45-120; teardown: src/cleanup.cpp:10-64).
 *
 * Plain pointers and sizes only; no C++/torch types.  Every function returns 0 on success or an MI_UNET_E* code and
 * leaves a human-readable message retrievable through mi_unet_last_error() (thread local).  There is no CPU fallback:
 * without a HIP device every entry point that needs one fails with MI_UNET_ENODEVICE.
 */
#ifndef MI_UNET_H
#define MI_UNET_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MI_UNET_OK 0
#define MI_UNET_EARG 1        /* bad argument / unsupported configuration */
#define MI_UNET_ENODEVICE 2   /* no usable HIP device */
#define MI_UNET_EHIP 3        /* a HIP runtime call failed (message carries hipGetErrorString) */
#define MI_UNET_EFILE 4       /* weight file missing / malformed / topology mismatch */
#define MI_UNET_ESTATE 5      /* call order violated (e.g. infer before load_weights) */

typedef struct mi_unet mi_unet_t;

typedef struct mi_unet_config {
    int height;      /* input tile height; the reference fixes 512 (src/process.cpp:70, :126) */
    int width;       /* input tile width;  512 */
    int in_ch;       /* 1 (grayscale, src/process.cpp:70) */
    int base;        /* channels of the first level, 64 */
    int levels;      /* number of 2x down/up steps, 4 */
    int classes;     /* 3 (src/process.cpp:162) */
    int max_batch;   /* images processed per micro-batch; device buffers are sized for this */
    int device;      /* HIP device ordinal (the reference uses implicit device 0) */
    int conv_algo;   /* 3x3 convolution algorithm, fp32 arithmetic on the fp32 MFMA unless stated:
                        MI_UNET_CONV_AUTO (environment MIUNET_CONV_ALGO=direct|winograd|winograd16|bf16|fp16, else the default),
                        MI_UNET_CONV_DIRECT (implicit GEMM, 9 taps), MI_UNET_CONV_WINOGRAD (the default: Winograd F(4x4,3x3), 4x
                        fewer MACs, on every layer whose grid fills the chip or can split K, F(2x2,3x3) on the rest; the
                        transposed convs as four per-tap GEMMs; head fused into the last conv.  DESIGN.md 4.2-4.4) */
} mi_unet_config;

#define MI_UNET_CONV_AUTO 0
#define MI_UNET_CONV_DIRECT 1
#define MI_UNET_CONV_WINOGRAD 2
#define MI_UNET_CONV_WINOGRAD16 3   /* same algorithm, 8-wave tiling on v_mfma_f32_16x16x4_f32 (two waves per SIMD) */
#define MI_UNET_CONV_BF16 4         /* BASELINE config 3: bf16 conv operands (weights packed bf16, activations rounded to
                                       bf16 once by the kernel that produces them and kept bf16 in HBM), fp32 accumulate on
                                       v_mfma_f32_16x16x32_bf16.  NOT the fp32 metric: logits follow the bf16-operand oracle. */
#define MI_UNET_CONV_FP16 5         /* BASELINE config 5's arithmetic: the same kernels with IEEE half operands
                                       (v_mfma_f32_16x16x32_f16), fp32 accumulate */
#define MI_UNET_CONV_DEFAULT MI_UNET_CONV_WINOGRAD

/* Fills *cfg with the reference's constants: 512x512x1, base 64, 4 levels, 3 classes, max_batch 16, device 0. */
void mi_unet_default_config(mi_unet_config *cfg);

/* Replaces createInferRuntime + per-thread context creation (src/initialize.cpp:48, src/process.cpp:45-120):
 * allocates all device buffers and the stream.  No weights yet. */
int mi_unet_create(const mi_unet_config *cfg, mi_unet_t **out);

/* Replaces reading + deserialising the .trt engine (src/initialize.cpp:49-60).  File format: miunet/spec.py
 * ("MIUNETW1").  Folds eval-mode BatchNorm into the conv weights, repacks for the MFMA kernels, uploads.
 * Version 1 files hold the transposed-conv decoder; version 2 files add a u32 up_mode after the header (0 = transposed 2x2,
 * 1 = bilinear x2 with align_corners=True, Pytorch-UNet's bilinear=True: halved bottleneck, narrower up convolutions).  The
 * decoder comes from the file, not from mi_unet_config; the buffers mi_unet_create allocates hold either plan.  An unknown
 * version or up_mode, or a payload whose length does not match the topology, is MI_UNET_EFILE. */
int mi_unet_load_weights(mi_unet_t *h, const char *path);
int mi_unet_load_weights_from_memory(mi_unet_t *h, const void *blob, size_t len);

/* The hot path = execute_inference (src/process.cpp:123-175) for B images at once, host buffers:
 *   imgs   u8  [B][H][W][in_ch]              (the 8-bit normalised tile the reference reads back at :217)
 *   labels u8  [B][H][W]          out        (class index per pixel, as pred_mask at :170)
 *   logits f32 [B][classes][H][W] out/NULL   (planar, the reference's output binding layout :81-85, :163)
 * B may exceed max_batch (processed in micro-batches). */
int mi_unet_infer_u8(mi_unet_t *h, const uint8_t *imgs, int B, uint8_t *labels, float *logits);

/* Same, with all three buffers already resident in device memory (HBM), 16-byte aligned; d_logits may be NULL.  The contract of the
 * device form:
 *  - Ordering.  The call enqueues on the handle's CURRENT stream -- the engine's own, or the one last given to mi_unet_set_stream --
 *    and returns without waiting.  It is ordered behind everything enqueued on that stream before it (a copy into d_imgs, say) and
 *    ahead of everything enqueued after it, as a kernel launch there would be; with mi_unet_set_postprocess on, the clean-up follows
 *    on the same stream.  Another stream, or the host, reads the results after mi_unet_sync() or after an event of that stream.
 *  - Buffers.  All three must stay valid, and d_imgs unchanged by anyone else, until the stream has passed the call.  Nothing outside
 *    B * H * W * in_ch bytes of d_imgs is read and nothing outside B * H * W bytes of d_labels and B * classes * H * W floats of
 *    d_logits is written.
 *  - B > max_batch.  The call walks the buffers in micro-batches: micro-batch k covers images [k * max_batch, min(B, (k + 1) *
 *    max_batch)), i.e. the contiguous slices d_imgs + k * max_batch * H * W * in_ch, d_labels + k * max_batch * H * W and d_logits +
 *    k * max_batch * classes * H * W, one behind the other on the stream.  B = 0 succeeds and enqueues nothing.
 *  - Graphs.  A micro-batch is keyed on (stream, its three slice pointers, its size).  The first call of a key launches kernel by
 *    kernel, the second captures those launches into a hipGraph, every later one replays it: the graph reads whatever the buffers hold
 *    when it runs.  The handle caches up to 64 keys and drops the oldest one first; before a dropped graph is destroyed the handle
 *    waits (on the host) for the work that may still replay it.  A caller that cycles through more than 64 keys (more than 64
 *    micro-batches in one call, or more than 64 buffer / stream combinations in turn) therefore never replays, and every call costs a
 *    kernel-by-kernel launch; keep the working set at 64 keys or raise max_batch.  MIUNET_GRAPH=0 and profiling launch kernel by
 *    kernel always.
 * One handle is driven by one host thread at a time; two handles (mi_unet_clone) on two streams run side by side. */
int mi_unet_infer_u8_device(mi_unet_t *h, const uint8_t *d_imgs, int B, uint8_t *d_labels, float *d_logits);

/* SURVEY §8f row f1 -- the arithmetic of Preprocess::preprocess_raw (src/preprocess.cpp:65-118) on the device, fused in
 * front of the network: B headerless little-endian u16 RAW images (host pointers; image i is heights[i] x widths[i]) ->
 * exact min/max -> top-left-aligned bilinear resample to the engine's H x W in fp64 -> u8 tiles (bit-exact with the
 * reference's CPU loop) -> UNet -> labels.  tiles (u8 [B][H][W][in_ch], host) and logits may be NULL.
 * Engines with in_ch = C > 1 (BASELINE config 5: C = 3) take C planes per image: raws / widths / heights then hold B*C
 * entries, plane c of image i at index i*C + c.  Every plane is preprocessed on its own (own size, own min/max -- exactly
 * what preprocess_raw would do to it as a file) and becomes channel c of the interleaved tile.  The reference defines only
 * single-plane RAW (src/preprocess.cpp:86); a caller holding one plane passes its pointer C times, which is the grey ->
 * B,G,R replication of cv::imread(IMREAD_COLOR) (src/mask2polygon.cpp:117). */
int mi_unet_infer_raw16(mi_unet_t *h, const uint16_t *const *raws, const int *widths, const int *heights, int B,
                        uint8_t *tiles, uint8_t *labels, float *logits);

/* SURVEY §8f row f2 -- postprocess_mask (src/postprocess.cpp:47-79) on the device, integer-exact: hole fill (8-connected
 * components of label != 2 that touch no image edge and are smaller than 6 % of the image), 3x3 open, keep components of
 * at least 6 % of the image; output in {0, 2}.
 *   mi_unet_set_postprocess(h, 1): every mi_unet_infer_* call returns the POSTPROCESSED masks instead of the raw label
 *                                  maps (the label maps never leave the device in between).
 *   mi_unet_postprocess_masks    : the stage alone on host buffers, u8 [B][H][W] in -> out (may alias). */
int mi_unet_set_postprocess(mi_unet_t *h, int on);
int mi_unet_postprocess_masks(mi_unet_t *h, const uint8_t *labels, int B, uint8_t *out);

/* SURVEY §8f row f3 -- Mask2Polygon::extract_contours (src/mask2polygon.cpp:29-36: threshold 127 +
 * findContours(RETR_EXTERNAL, CHAIN_APPROX_SIMPLE)) on the device, same point sequences and contour order.
 *   masks  u8 [B][H][W] host (e.g. the 0/128/255 visualisation of mask_to_image; > 127 = foreground)
 *   xy     int32 [B][cap_points][2] out: x,y pairs of image b's contours, contour after contour (newest first)
 *   start  int32 [B][cap_contours + 1] out: first point of contour c; entry [counts[b]] = total points of image b
 *   counts int32 [B] out: number of contours of image b, or -1 if one of the two capacities was too small for it */
int mi_unet_extract_contours(mi_unet_t *h, const uint8_t *masks, int B, int32_t *xy, int cap_points, int32_t *start,
                             int cap_contours, int32_t *counts);

/* The whole device half of process_single_image (src/process.cpp:188-242) for B images in one call, nothing leaving the
 * device in between: RAW16 -> min/max + bilinear + quantise (f1) -> UNet + argmax -> postprocess_mask (f2) ->
 * mask_to_image -> extract_contours (f3).  Outputs (host): tiles u8 [B][H][W] (the _normalized.png pixels, may be NULL),
 * masks u8 [B][H][W] (the _mask.png pixels: 0 / 255), and the contours in the layout of mi_unet_extract_contours. */
int mi_unet_segment_raw16(mi_unet_t *h, const uint16_t *const *raws, const int *widths, const int *heights, int B,
                          uint8_t *tiles, uint8_t *masks, int32_t *xy, int cap_points, int32_t *start, int cap_contours,
                          int32_t *counts);

/* ---- Tiled inference: one image LARGER than the engine's tile, segmented at its own resolution ---------------------------
 * The entry points above run images of exactly height x width; larger RAW images are resampled down to that size first (the
 * reference's behaviour, and the default).  The tiled forms instead cut one image of H x W (H >= height, W >= width) into
 * overlapping tiles of the engine's size on the device, run them in tile order in micro-batches of max_batch, and stitch the
 * per-tile label maps (and logits) back into one H x W result before anything else happens to it.
 *
 * The grid, per axis (image length L, tile length T, halo h; L >= T, h >= 0, 2h < T):
 *     S = T - 2h;  n = 1 + ceil((L - T) / S);  origin o_k = min(k S, L - T)   (the last tile ends at the image edge)
 *     cuts c_0 = 0, c_n = L, c_k = (o_{k-1} + T + o_k) / 2;  tile k owns positions [c_k, c_{k+1})
 * Tiles are numbered row-major (t = ty * nx + tx).  mi_unet_tile_axis returns n and, where the pointers are not NULL,
 * origins[n] and cuts[n + 1]; -1 for an illegal (L, T, halo).  Pure host arithmetic, needs no device.
 *
 * What the halo promises: a tile border that is an image border is the network's own zero padding, and every owned pixel lies
 * at least `halo` pixels inside every other tile border.  What it does not: a pixel of the default 4-level network sees roughly a
 * hundred pixels to every side (two 3x3 convolutions per level at strides 1 .. 16, down and up), and with a halo smaller than
 * that receptive field the tiled result is NOT the result of one pass over the whole image.  By default the result is exactly defined as "each pixel from the tile that owns it": equal, bit
 * for bit, to mi_unet_infer_u8 on the same tiles stacked in tile order followed by a copy of the owned rectangles.  No blending
 * (MI_UNET_BLEND_OWNER without mirrors); the tile blend setting below replaces the copy with a weighted mean of the overlapping tiles.
 *
 *   mi_unet_infer_tiled_u8    : img u8 [H][W][in_ch] (host) -> labels u8 [H][W], logits f32 [classes][H][W] or NULL
 *   mi_unet_infer_tiled_raw16 : in_ch planes of u16 [H][W] (argument order W, H as in mi_unet_infer_raw16; a caller holding one
 *                               plane passes its pointer in_ch times) -> exact min/max per plane and the quantisation of
 *                               mi_unet_infer_raw16 WITHOUT resampling -> norm u8 [H][W][in_ch] (may be NULL) -> as above
 *   mi_unet_segment_tiled_raw16 : ... -> postprocess_mask -> mask_to_image -> extract_contours, all on the stitched image:
 *                               mask u8 [H][W] (0 / 255), contours in the layout of mi_unet_extract_contours with B = 1, points in
 *                               full-image coordinates (no rescaling); *count = -1 when a capacity was too small
 * mi_unet_set_postprocess(h, 1) applies to the infer_tiled forms on the STITCHED image: one image, min_area = 6 % of H x W, never
 * per tile.  The postprocess and contour stages borrow the network's scratch buffer (4 * max_batch * height * width * base bytes);
 * an image whose workspace exceeds it fails with MI_UNET_EARG before anything runs.  Also MI_UNET_EARG: null pointers,
 * H < height, W < width, halo < 0, 2 * halo >= min(height, width); MI_UNET_ESTATE before weights are loaded.
 * The image is uploaded once; its full-size device buffers belong to the handle (a clone owns its own), grow on demand and are
 * freed by mi_unet_destroy.  mi_unet_last_stage_ms covers these calls: upload + min/max + normalise + gather in UPLOAD_PRE,
 * network + stitch in NETWORK, the rest as named. */
int mi_unet_tile_axis(int L, int T, int halo, int *origins, int *cuts);
int mi_unet_infer_tiled_u8(mi_unet_t *h, const uint8_t *img, int H, int W, int halo, uint8_t *labels, float *logits);
int mi_unet_infer_tiled_raw16(mi_unet_t *h, const uint16_t *const *planes, int W, int H, int halo, uint8_t *norm, uint8_t *labels,
                              float *logits);
int mi_unet_segment_tiled_raw16(mi_unet_t *h, const uint16_t *const *planes, int W, int H, int halo, uint8_t *norm, uint8_t *mask,
                                int32_t *xy, int cap_points, int32_t *start, int cap_contours, int32_t *count);

/* ---- Tile blending and mirror averaging: a per-handle setting that all three tiled entry points obey ------------
 * The default { MI_UNET_BLEND_OWNER, 0.125, 0 } is the ownership stitch above, unchanged bit for bit.  Any other setting runs:
 *   views   : each tile has nv views, in this order: identity; X if mirror & MI_UNET_MIRROR_X; Y if mirror & MI_UNET_MIRROR_Y; XY if
 *             mirror == 3.  View images run through the network in the order k = t * nv + v (t = the row-major tile index), in
 *             micro-batches of max_batch taken over k.  A view image is the tile cut at its origin and then mirrored (X: column j
 *             <- tw - 1 - j; Y: row i <- th - 1 - i); its logits are mirrored back before use.
 *   weights : the table of one axis of length T (mi_unet_tile_blend_weights), computed in double and rounded to float once:
 *             CONSTANT (and OWNER) w(i) = 1;  GAUSSIAN w(i) = max(exp(-(d * d) / (2 s s)), 2^-20), d = i - (T - 1) / 2,
 *             s = sigma_scale * T.  The floor keeps the 2-D product normal; the table is symmetric bit for bit.
 *             A view of tile (ty, tx) with origin (oy, ox) weighs image pixel (Y, X) with w = fl32(wy[Y - oy] * wx[X - ox])
 *             (wy: the table of the tile height, wx: of the tile width).
 *   sum     : per pixel and class, over the views that cover the pixel in increasing k: acc = fl32(acc + fl32(w * logit)) from +0,
 *             wsum = fl32(wsum + w) in the same order; no fused multiply-add.  The order is fixed by k, not by the micro-batches.
 *   result  : logit = acc / wsum, correctly rounded; label = the first-max-wins argmax of those logits (as the untiled head).
 *   OWNER with mirror != 0: only the owning tile's views contribute, with w = 1: their mean.
 * The logits of every view are computed (the network always writes logits in these modes) and accumulated on the device in a
 * full-size fp32 buffer of the handle; postprocessing and the segment form's tail run on the blended label map.
 * mi_unet_last_stage_ms: gather in UPLOAD_PRE, network + tile_blend + blend_finalize in NETWORK.
 * MI_UNET_EARG, setting unchanged: an unknown mode, a mirror outside 0..3, for GAUSSIAN a sigma_scale that is not finite or <= 0.
 * b == NULL restores the default.  A clone starts at the default. */
#define MI_UNET_BLEND_OWNER 0      /* default: each pixel from the tile that owns it */
#define MI_UNET_BLEND_CONSTANT 1   /* plain mean over every view that covers the pixel */
#define MI_UNET_BLEND_GAUSSIAN 2   /* weighted mean, separable Gaussian importance map centred on each tile */
#define MI_UNET_MIRROR_X 1         /* also run each tile mirrored left-right */
#define MI_UNET_MIRROR_Y 2         /* ... and/or top-bottom (both: 4 views including the XY mirror) */
typedef struct mi_unet_tile_blend {
    int mode;            /* MI_UNET_BLEND_* */
    float sigma_scale;   /* GAUSSIAN: sigma as a fraction of the tile length (0.125 = nnU-Net's 1/8) */
    int mirror;          /* MI_UNET_MIRROR_* bits, 0..3 */
} mi_unet_tile_blend;
int mi_unet_set_tile_blend(mi_unet_t *h, const mi_unet_tile_blend *b);
int mi_unet_get_tile_blend(const mi_unet_t *h, mi_unet_tile_blend *b);
/* Pure host arithmetic, needs no device: the weight table of one axis (w[T]) that the kernels use for the setting *b; MI_UNET_EARG for
 * T < 1, null pointers or an invalid setting. */
int mi_unet_tile_blend_weights(int T, const mi_unet_tile_blend *b, float *w);

/* ---- Targets: which classes the tail segments, and how small a structure may be ---------------------------------
 * A target is a class and its area rule.  Its mask is postprocess_mask (above) with `== cls` in place of `== 2` and min_area_frac in
 * place of 6 %: fill the 8-connected components of label != cls whose bounding box touches no image edge and whose area is below
 * min_area, open 3x3 (the border neither constrains nor seeds), keep the 8-connected components of at least min_area pixels.
 * min_area = mi_unet_target_min_area(H, W, min_area_frac) = (int)((float)(W * H) * min_area_frac): the int product converted to float
 * and multiplied in float, so 0.06f gives the numbers of the single-class entry points (pure host arithmetic, needs no device).
 * Targets are independent: after hole filling two of them may claim the same pixel.
 * The setting is per handle.  Default { { 2, 0.06f } }; t == NULL or n == 0 restores it; a clone starts at the default.
 * MI_UNET_EARG, setting unchanged: n < 0 or n > MI_UNET_MAX_TARGETS, cls < 1 or cls >= classes, a repeated cls, a min_area_frac that is
 * not finite or lies outside [0, 1].  mi_unet_get_targets writes min(*n, cap) entries and the number of targets to *n.
 * Only the _multi entry points read the setting; every other entry point -- mi_unet_set_postprocess included -- keeps class 2 and 6 %.
 * With K = the number of targets, in target order:
 *   mi_unet_postprocess_masks_multi   : labels u8 [B][H][W] (host) -> out u8 [B][K][H][W], values in {0, cls_k}
 *   mi_unet_segment_raw16_multi       : mi_unet_segment_raw16 with masks u8 [B][K][H][W] (0 / 255), xy [B][K][cap_points][2],
 *                                       start [B][K][cap_contours + 1], counts [B][K]; -1 marks only the (image, target) whose capacity
 *                                       was too small
 *   mi_unet_segment_tiled_raw16_multi : mi_unet_segment_tiled_raw16 with mask u8 [K][H][W], xy [K][cap_points][2],
 *                                       start [K][cap_contours + 1], count [K]; min_area from the full image.  MI_UNET_EARG before
 *                                       anything runs when the K-fold workspace exceeds the borrowed scratch buffer.
 * The (image, target) pairs run as B * K independent planes through the same launches as one target; the label map is read in place.
 * The RAW form's workspace and output buffers grow on demand and belong to the handle.  With the default setting every _multi call
 * returns exactly the bytes of its single-class counterpart.  mi_unet_last_stage_ms covers these calls under the same stage names. */
#define MI_UNET_MAX_TARGETS 5
typedef struct mi_unet_target {
    int cls;               /* class index, 1 .. classes - 1 */
    float min_area_frac;   /* smallest structure kept / largest hole filled, as a fraction of the image area, in [0, 1] */
} mi_unet_target;
int mi_unet_target_min_area(int H, int W, float frac);
int mi_unet_set_targets(mi_unet_t *h, const mi_unet_target *t, int n);
int mi_unet_get_targets(const mi_unet_t *h, mi_unet_target *t, int cap, int *n);
int mi_unet_postprocess_masks_multi(mi_unet_t *h, const uint8_t *labels, int B, uint8_t *out);
int mi_unet_segment_raw16_multi(mi_unet_t *h, const uint16_t *const *raws, const int *widths, const int *heights, int B,
                                uint8_t *tiles, uint8_t *masks, int32_t *xy, int cap_points, int32_t *start, int cap_contours,
                                int32_t *counts);
int mi_unet_segment_tiled_raw16_multi(mi_unet_t *h, const uint16_t *const *planes, int W, int H, int halo, uint8_t *norm, uint8_t *mask,
                                      int32_t *xy, int cap_points, int32_t *start, int cap_contours, int32_t *count);

/* ---- Morphology: the element of a target's clean-up, so that it can scale with the image -------------------------------
 * The reference's third tunable, MORPH_KERNEL_SIZE (src/postprocess.cpp), per target: a radius for the opening, an optional closing in
 * front of it and a choice of box or Euclidean disc.  The element of radius r is (2r + 1) x (2r + 1) with its anchor at the centre:
 *   MI_UNET_MORPH_RECT : every (dx, dy) with |dx| <= r and |dy| <= r, = cv::getStructuringElement(MORPH_RECT, (2r + 1, 2r + 1))
 *   MI_UNET_MORPH_DISC : { (dx, dy) : dx*dx + dy*dy <= r*r }, in integer arithmetic (r = 1 is the plus)
 * mi_unet_morph_element writes it as (2r + 1) * (2r + 1) bytes 0 / 1, row after row (pure host arithmetic, needs no device);
 * MI_UNET_EARG for an unknown shape, r outside 0 .. MI_UNET_MORPH_MAX_R or a null pointer.
 * With a morphology a target's mask is four steps:
 *   1. fill holes (as above, unchanged)
 *   2. close : dilate by the element of radius close_r, then erode by it
 *   3. open  : erode by the element of radius open_r, then dilate by it
 *   4. area filter (as above, unchanged)
 * Border rules for every radius and both shapes: an erosion is constrained only by pixels inside the image (a pixel survives when every
 * element position that falls inside the image is foreground), a dilation is seeded only by pixels inside the image.  r = 0 is the
 * identity; { RECT, 1, 0 } is the reference's 3x3 open.  Integer-exact like the rest of the tail.
 * The setting is per handle and off by default: { { RECT, 1, 0 } }.  mi_unet_set_morph: n = 1 applies the entry to every target, n = K
 * gives one entry per target in target order; m == NULL or n == 0 restores the default; a clone starts at the default.  MI_UNET_EARG,
 * setting unchanged: an unknown shape, a radius outside 0 .. MI_UNET_MORPH_MAX_R, n < 0 or n > MI_UNET_MAX_TARGETS.  The list is not tied
 * to the targets when it is set and mi_unet_set_targets does not touch it: a _multi call whose stored list is longer than 1 and not as
 * long as its target list fails with MI_UNET_ESTATE and a message before anything is queued.  mi_unet_get_morph writes min(*n, cap)
 * entries and the number stored to *n.
 * Only the _multi entry points read the setting (mi_unet_postprocess_masks_multi, mi_unet_segment_raw16_multi,
 * mi_unet_segment_tiled_raw16_multi, mi_unet_group_segment_raw16_multi); every other entry point -- mi_unet_set_postprocess included --
 * keeps the 3x3 box.  With the default setting every call enqueues exactly the launches it enqueued before and returns the same bytes.
 * On the tiled route the tail runs at the image's native resolution: scale the radius with native / tile resolution to reproduce the
 * clean-up of the resampled route (min_area already scales, being a fraction).  The time counts under MI_UNET_STAGE_POSTPROCESS. */
#define MI_UNET_MORPH_RECT 0     /* (2r+1) x (2r+1) box: cv::getStructuringElement(MORPH_RECT) */
#define MI_UNET_MORPH_DISC 1     /* { (dx, dy) : dx*dx + dy*dy <= r*r }, integer arithmetic */
#define MI_UNET_MORPH_MAX_R 31
typedef struct mi_unet_morph { int shape; int open_r; int close_r; } mi_unet_morph;   /* default { RECT, 1, 0 } */
int mi_unet_set_morph(mi_unet_t *h, const mi_unet_morph *m, int n);
int mi_unet_get_morph(const mi_unet_t *h, mi_unet_morph *m, int cap, int *n);
int mi_unet_morph_element(int shape, int r, uint8_t *elem /* [(2r+1)*(2r+1)], 0 / 1 */);

/* ---- Intensity windows: which sample range of a RAW16 plane becomes 0..255 ---------------------------------------
 * A per-handle setting that every RAW-in entry point reads (mi_unet_infer_raw16, mi_unet_segment_raw16{,_multi},
 * mi_unet_infer_tiled_raw16, mi_unet_segment_tiled_raw16{,_multi} and their group forms).  The default, MINMAX, is the reference's
 * stretch of the exact minimum and maximum, unchanged bit for bit.  One hot or dead pixel sets that window; the other two modes do
 * not depend on single samples.
 * The window is per plane (every plane of an in_ch > 1 image has its own, as it has its own min / max; a pointer passed in_ch times
 * is scanned once).  With the plane's n samples sorted ascending as s[0 .. n - 1]:
 *   PERCENTILE : k_lo = floor(n * clip_lo_ppm / 1000000), k_hi = floor(n * clip_hi_ppm / 1000000) in 64-bit integers;
 *                lo = s[k_lo], hi = s[n - 1 - k_hi].  Exact (a radix select on the device), never an estimate; 0, 0 ppm is min / max.
 *   FIXED      : lo, hi as given; nothing is scanned.
 * Quantisation in these two modes, for the resampling and the tiled path alike: L = lo, Hh = hi if hi > lo else lo + 1 (in int, no
 * wrap), v = the sample or the fp64 bilinear interpolant of the min/max path, vc = min(max(v, L), Hh),
 * byte = (uint8_t)(int)((vc - L) * (255.0 / (Hh - L)) + 0.5), every operation rounded once.  PERCENTILE at 0, 0 ppm returns the
 * bytes of MINMAX.  Planes of 2^32 samples or more are refused with MI_UNET_EARG in PERCENTILE mode.
 * MI_UNET_EARG, setting unchanged: an unknown mode; PERCENTILE with a negative ppm or clip_lo_ppm + clip_hi_ppm >= 1000000; FIXED
 * outside 0 <= lo < hi <= 65535.  Fields the mode does not use are ignored.  w == NULL restores the default; a clone starts at the
 * default.  mi_unet_group_set_window changes every rank or none.
 * mi_unet_window_of is the definition as pure host arithmetic (needs no device): the window of n samples under *w.
 * mi_unet_last_windows: the windows the LAST RAW-in call on this handle applied, one (lo, hi) pair per plane in call order (B * in_ch
 * planes; tiled: in_ch), as found -- before the lo + 1 bump; in MINMAX mode the min / max.  Writes min(count, cap) pairs and the
 * count to *n; MI_UNET_ESTATE before any RAW-in call has completed.  The selection counts under MI_UNET_STAGE_UPLOAD_PRE. */
#define MI_UNET_WINDOW_MINMAX     0   /* default: the reference's min/max stretch, unchanged bit for bit */
#define MI_UNET_WINDOW_PERCENTILE 1   /* clip a share of the samples at each end */
#define MI_UNET_WINDOW_FIXED      2   /* the caller's lo..hi */
typedef struct mi_unet_window {
    int mode;
    int clip_lo_ppm, clip_hi_ppm;   /* PERCENTILE: samples clipped at the dark / bright end, parts per million of the plane */
    int lo, hi;                     /* FIXED: 0 <= lo < hi <= 65535 */
} mi_unet_window;
int mi_unet_set_window(mi_unet_t *h, const mi_unet_window *w);
int mi_unet_get_window(const mi_unet_t *h, mi_unet_window *w);
int mi_unet_window_of(const uint16_t *samples, size_t n, const mi_unet_window *w, int *lo, int *hi);
int mi_unet_last_windows(const mi_unet_t *h, int32_t *lo_hi, int cap, int *n);

/* ---- Region measurement: area, moments and intensity of every contoured region, on the device ---------------------
 * A per-handle setting, off by default; with it off every call does exactly what it did before.
 * A REGION is an 8-connected component of the contour stage's foreground (mask > 127) that has an external contour.  Components nested
 * inside a hole of another component get no contour under RETR_EXTERNAL, so they get no region.  Region c of plane p describes exactly
 * contour c of plane p: the order is the same, and the region's raster-first pixel is the contour's first point.  A plane is an image,
 * or an (image, target) pair, in the same [B][K] order as the contour outputs.  Coordinates are those of the mask the contour stage saw:
 * tile coordinates for the RAW forms, full-image coordinates for the tiled forms.
 * All fields are integers and all are exact.  None of the sums can overflow for any input the tail accepts: planes x H x W < 2^31
 * gives sxx < 2^62.  (Exactly: sxx < H W^3 / 3, syy < W H^3 / 3 and sxy between them, all below H W max(H, W)^2 / 3, which stays under
 * 2^62 for every image of up to 2^31 pixels whose longer side is below 80264 pixels.  A measuring call on a mask with
 * H W max(H, W)^2 >= 3 x 2^62 is refused with MI_UNET_EARG before anything runs.)
 * With mi_unet_measure.on set, every entry point that returns contours also measures: mi_unet_segment_raw16{,_multi},
 * mi_unet_segment_tiled_raw16{,_multi} and the group forms.  The measured channel is `channel` of the normalised tile the network read
 * (tiled forms: of the full-size normalised image); plane b * K + k reads image b.
 * mi_unet_last_regions serves the LAST such call on the handle: *planes and *cap_contours describe the call (regions and counts may be
 * NULL to query them); regions is [min(planes, cap_planes)][cap_contours]; counts[p] is the number of external components of plane p, or
 * -1 when it exceeded cap_contours.  counts[p] does not depend on cap_points: a plane whose points overflowed still has valid regions.
 * Entries at c >= counts[p], and every entry of a -1 plane, are all-zero.  MI_UNET_ESTATE when the last contour-returning call did not
 * measure, or when there was none.  mi_unet_set_measure: MI_UNET_EARG, setting unchanged, for a channel outside 0 .. in_ch - 1; NULL
 * restores the default { 0, 0 }; a clone starts at the default.
 * mi_unet_measure_regions is the stage alone, the counterpart of mi_unet_extract_contours with the same preconditions, on host buffers:
 * masks u8 [B][H][W], tiles u8 [B][H][W][in_ch] or NULL, regions [B][cap_contours] out, counts [B] out.  With tiles == NULL:
 * imin = imax = 0, si = sii = 0, channel = -1.  It does not change what mi_unet_last_regions reports.
 * mi_unet_region_derive is pure host arithmetic (needs no device); MI_UNET_EARG for area < 1 or a null pointer.  With A = area:
 *   cx = sx / A and cy = sy / A.
 *   The central second moments have exact 128-bit integer numerators that are converted once: m20 = (A*sxx - sx^2) / A^2, m02 likewise,
 *   m11 = (A*sxy - sx*sy) / A^2.
 *   a = m20 + 1/12, c = m02 + 1/12 (a pixel is a unit square), b = m11.
 *   lambda+- = ((a + c) +- sqrt((a - c)^2 + 4 b^2)) / 2.
 *   major = 4 sqrt(lambda+) and minor = 4 sqrt(lambda-): the axes of the ellipse with the same second moments.  One pixel gives 1.1547
 *   for both.
 *   theta = 0.5 atan2(2 b, a - c): the angle of the major axis from +x, with y pointing down.
 *   mean = si / A and std = sqrt((A*sii - si^2) / A^2).
 * The time of the measurement counts under MI_UNET_STAGE_CONTOURS. */
typedef struct mi_unet_region {      /* 96 bytes, no padding */
    int32_t area;                    /* pixels of the component; holes are not counted */
    int32_t x0, y0, x1, y1;          /* bounding box, inclusive */
    int32_t imin, imax;              /* min / max of the measured channel of the normalised tile over the component */
    int32_t channel;                 /* the channel measured (echo of the setting; -1 when no tile was given) */
    int64_t edges;                   /* crack perimeter: pixel edges between a component pixel and a 4-neighbour that is
                                        not foreground; the image frame counts as not foreground; hole borders count */
    int64_t sx, sy;                  /* sum of x, sum of y over the component */
    int64_t sxx, syy, sxy;           /* sum of x*x, y*y, x*y */
    int64_t si, sii;                 /* sum of v, sum of v*v, with v = the tile byte of the measured channel */
} mi_unet_region;
typedef struct mi_unet_measure { int on; int channel; } mi_unet_measure;   /* default {0, 0}; channel in 0 .. in_ch-1 */
typedef struct mi_unet_region_shape { double cx, cy, mean, std, major, minor, theta; } mi_unet_region_shape;
int mi_unet_set_measure(mi_unet_t *h, const mi_unet_measure *m);           /* NULL restores the default; a clone starts at it */
int mi_unet_get_measure(const mi_unet_t *h, mi_unet_measure *m);
int mi_unet_last_regions(const mi_unet_t *h, mi_unet_region *regions, int32_t *counts, int cap_planes,
                         int *planes, int *cap_contours);
int mi_unet_measure_regions(mi_unet_t *h, const uint8_t *masks, const uint8_t *tiles /* [B][H][W][in_ch] or NULL */,
                            int B, int channel, mi_unet_region *regions, int cap_contours, int32_t *counts);
int mi_unet_region_derive(const mi_unet_region *r, mi_unet_region_shape *out);   /* EARG for area < 1 or NULL */

/* ---- Scores against ground truth: overlap and surface distance per class, on the device ---------------------------
 * A stage of its own, not a setting: nothing else in this header changes behaviour because of it.
 * Inputs are two byte maps pred and truth, each u8 [B][H][W], and n byte values, 1 <= n <= MI_UNET_SCORE_MAX_VALUES.  H and W are
 * arguments, not the engine's tile size (tiled results are full-size).  Plane (b, k) compares the sets A = { pred == values[k] } and
 * T = { truth == values[k] } of image b.  That covers label maps (values = class indices), the {0, cls} masks of the tail
 * (values = { cls }) and 0 / 255 pictures (values = { 255 }, the truth coded alike).
 *   OVERLAP   tp = |A n T|, fp = |A \ T|, fn = |T \ A|.  Always valid.
 *   BOUNDARY  dS = every pixel of S with a 4-neighbour that is not in S; positions outside the image are not in S, so a set that
 *             touches the frame has boundary there (the frame rule of mi_unet_region.edges).  It is S & ~binary_erosion(S) with
 *             scipy's default cross and border_value = 0: the surface medpy measures.
 *   DISTANCE  between pixel centres, kept SQUARED, in integers, no radius cap: for p in dA, d2(p) = min over q in dT of |p - q|^2
 *             (direction a_to_t), and likewise from dT to dA (t_to_a).  Per direction: n = boundary pixels of the source set,
 *             max_d2 = the directed Hausdorff distance squared, sum_d2 = the sum of d2, sum_d_q16 = the sum of floor(2^16 sqrt(d2)),
 *             every term the exact integer floor (an integer square root of d2 << 32), so the sum does not depend on the order of
 *             addition and is bit-reproducible.
 *   ORDER STATISTIC  by the convention of the window section: with the direction's n values sorted ascending as s[0 .. n - 1] and
 *             k = floor(n * quantile_ppm / 1000000) in 64-bit integers, q_d2 = s[n - 1 - k].  0 ppm is max_d2; 50000 is the "HD95" cut.
 *             q_d2_sym is the same statistic over both directions' values together (n = n_a + n_t): the multiset medpy's hd95 takes
 *             its percentile over.  It is an ORDER STATISTIC, exact, found by a radix select -- never an interpolated percentile:
 *             numpy.percentile interpolates between neighbours and can differ from it by up to their gap.
 *   EMPTY     when dA or dT is empty both n fields still hold the counts, every max_d2, q_d2 and q_d2_sym is -1 and the sums are 0.
 * Limits: H, W in 1 .. 32767 (so d2 <= 2 * 32766^2 < 2^31), B * n * H * W < 2^31 and B * n <= MI_UNET_SCORE_MAX_PLANES = 32767 planes in
 * one call (the device form numbers its workgroups per plane and row in 31 bits).  No field can overflow under them: a direction has
 * at most H * W < 2^30 values (H * W <= B * n * H * W), so sum_d2 < 2^30 * 2^31 = 2^61 and sum_d_q16 < 2^30 * 2^16 * 2^15.5 < 2^62.
 * The confusion matrix (optional; opts->classes in 1 .. MI_UNET_SCORE_MAX_CLASSES, confusion and skipped not NULL): int64 [B][classes][classes], row = the
 * truth byte, column = the pred byte; pixels where either byte is >= classes are left out of it and counted in int64 skipped[B], so
 * an image's entries plus its skipped always sum to H * W.
 * mi_unet_score_labels takes host buffers, like mi_unet_measure_regions; its workspace grows on demand and belongs to the handle.  It
 * needs the device, not the network: it works before weights are loaded.  It changes no setting and nothing mi_unet_last_regions or
 * mi_unet_last_stage_ms report.  opts == NULL is { 50000, 0 }.  MI_UNET_EARG with a message, nothing queued and no output written: a
 * null pred, truth, values or scores; B < 1; n outside 1 .. MI_UNET_SCORE_MAX_VALUES; a value outside 0 .. 255 or repeated;
 * quantile_ppm outside 0 .. 999999; classes outside 0 .. 16; more than MI_UNET_SCORE_MAX_PLANES planes; confusion given with classes == 0 or without skipped; H, W or
 * B * n * H * W outside the limits.  confusion == NULL skips the matrix whatever classes says.
 * mi_unet_score_labels_host is the definition as pure host arithmetic (needs no device), same arguments without the handle, same bytes.
 * mi_unet_score_derive is pure host arithmetic; MI_UNET_EARG for a null pointer.  A ratio whose denominator is 0 is 1 -- nothing was
 * there and nothing was claimed, a perfect score -- for all four:
 *   dice = 2 tp / (2 tp + fp + fn), iou = tp / (tp + fp + fn), precision = tp / (tp + fp), recall = tp / (tp + fn);
 *   hd = sqrt(max(a_to_t.max_d2, t_to_a.max_d2)), hd_q = sqrt(q_d2_sym);
 *   assd = (a_to_t.sum_d_q16 + t_to_a.sum_d_q16) / 65536 / (n_a + n_t), rmsd = sqrt((a_to_t.sum_d2 + t_to_a.sum_d2) / (n_a + n_t)).
 * The four distance metrics are NaN when the distance fields are -1.
 * There is no group form: mi_unet_group_handle(g, rank) hands out an engine to call this on. */
#define MI_UNET_SCORE_MAX_VALUES 8
#define MI_UNET_SCORE_MAX_CLASSES 16
#define MI_UNET_SCORE_MAX_PLANES 32767
typedef struct mi_unet_score_dir {   /* 32 bytes, no padding */
    int32_t n;                       /* boundary pixels of the source set */
    int32_t max_d2;                  /* directed Hausdorff distance, squared; -1 when either boundary is empty */
    int32_t q_d2;                    /* the order statistic of the direction's d2 values; -1 likewise */
    int32_t reserved;                /* 0 */
    int64_t sum_d2;                  /* sum of d2 */
    int64_t sum_d_q16;               /* sum of floor(2^16 sqrt(d2)) */
} mi_unet_score_dir;
typedef struct mi_unet_score {       /* 88 bytes, no padding */
    int32_t tp, fp, fn;
    int32_t q_d2_sym;                /* the order statistic over both directions' values together; -1 when either boundary is empty */
    int32_t value, quantile_ppm;     /* echo of the plane's value and of the call's quantile */
    mi_unet_score_dir a_to_t, t_to_a;
} mi_unet_score;
typedef struct mi_unet_score_opts { int quantile_ppm; int classes; } mi_unet_score_opts;   /* default { 50000, 0 }; classes = 0: no matrix */
typedef struct mi_unet_score_metrics { double dice, iou, precision, recall, hd, hd_q, assd, rmsd; } mi_unet_score_metrics;
int mi_unet_score_labels(mi_unet_t *h, const uint8_t *pred, const uint8_t *truth, int B, int H, int W, const int *values, int n,
                         const mi_unet_score_opts *opts, mi_unet_score *scores /* [B][n] */, int64_t *confusion, int64_t *skipped);
int mi_unet_score_labels_host(const uint8_t *pred, const uint8_t *truth, int B, int H, int W, const int *values, int n,
                              const mi_unet_score_opts *opts, mi_unet_score *scores /* [B][n] */, int64_t *confusion, int64_t *skipped);
int mi_unet_score_derive(const mi_unet_score *s, mi_unet_score_metrics *out);

/* ---- Volume components: a stack of masks labelled as one volume, size filter, volumetry -----------------------------
 * A stage of its own, not a setting: nothing else in this header changes behaviour because of it.
 * Input is one byte volume masks, u8 [D][H][W] (slice z, row y, column x; D, H, W are arguments, not the engine's tile size), and n
 * byte values, 1 <= n <= MI_UNET_VOLUME_MAX_VALUES.  Plane k is the set S = { masks == values[k] } of the volume; planes are independent.
 *   ADJACENCY  two voxels of S are adjacent when they differ by at most 1 on every axis and, connectivity 6: on exactly one axis;
 *              18: on at most two axes; 26: on up to three.  A component is a maximal connected subset of S.  With D = 1, connectivity 6
 *              is the 2-D 4-connectivity and 18 / 26 are the 8-connectivity.
 *   FIELDS     per component: voxels; first = its raster-first voxel, z * H * W + y * W + x; the inclusive bounding box; sx, sy, sz = the
 *              sums of x, y, z over its voxels; faces_x / _y / _z = the voxel faces perpendicular to that axis between a voxel of the
 *              component and a 6-neighbour that is not in S.  Positions outside the volume are not in S (the frame rule of
 *              mi_unet_region.edges), and the walls of a closed cavity count.  Every 6-neighbour in S belongs to the same component under
 *              all three connectivities, so "not in S" is the same as "not in the component".
 *   ORDER      the components of a plane are ordered by voxels descending, ties by first ascending; first is unique, so the order is
 *              total.  As one integer the key is (voxels << 31) | (2^31 - 1 - first), descending.
 *   FILTER     the component at position r of that order is kept iff voxels >= min_voxels and (keep_largest == 0 or r < keep_largest).
 *              out [n][D][H][W] is values[k] where the voxel's component is kept and 0 elsewhere; it may be masks itself when n == 1,
 *              and may be NULL.  The filter never depends on cap.
 *   COUNTS     found[k] = the components of the plane, kept[k] = the number kept; both always exact, whatever cap is.
 *   TABLE      table[k] ([n][cap]) holds the first min(found, cap) components in the order above; the entries behind them are all-zero.
 *   IDS        ids [n][D][H][W] (or NULL) holds per voxel: 1 + the table index of a kept component that is in the table; -1 for a voxel
 *              of a kept component that did not fit; 0 everywhere else.
 * Limits: D, H, W >= 1; n * D * H * W < 2^31, so every index is an int, sx < 2^62 and a face count is at most 6 * 2^31; values in
 * 0 .. 255 and not repeated; cap in 1 .. MI_UNET_VOLUME_MAX_TABLE; connectivity in { 6, 18, 26 }; min_voxels >= 0; keep_largest >= 0.
 * opts == NULL is { 26, 0, 0 }.
 * mi_unet_volume_components takes host buffers of any size; its workspace grows on demand, belongs to the handle and is freed by
 * mi_unet_destroy.  It needs the device, not the network: it works before weights are loaded.  It changes no setting and nothing
 * mi_unet_last_regions or mi_unet_last_stage_ms report.  MI_UNET_EARG with a message, nothing queued and no output written: a null
 * masks, values, table, found or kept; D, H or W < 1; n outside 1 .. MI_UNET_VOLUME_MAX_VALUES; a value outside 0 .. 255 or repeated;
 * n * D * H * W >= 2^31; cap outside 1 .. MI_UNET_VOLUME_MAX_TABLE; a connectivity other than 6, 18, 26; min_voxels < 0; keep_largest < 0.
 * A workspace that cannot be allocated is MI_UNET_EHIP with a message, before anything runs; the handle stays usable.
 * mi_unet_volume_components_host is the definition as pure host arithmetic (needs no device), same arguments without the handle, same
 * bytes.
 * mi_unet_volume_derive is pure host arithmetic: MI_UNET_EARG for a null pointer, voxels < 1, or a spacing that is not finite and > 0.
 * A voxel is a box of spacing_xyz[0] x [1] x [2] millimetres and voxel 0 spans 0 .. 1 of the grid:
 *   volume_mm3 = voxels * sx * sy * sz;  surface_mm2 = faces_x * sy * sz + faces_y * sx * sz + faces_z * sx * sy (s = the spacing);
 *   c*_mm = (sum / voxels + 0.5) * spacing of the axis;  extent_*_mm = (hi - lo + 1) * spacing of the axis.
 * The surface is that of the voxel boxes (a crack surface): it overestimates the smooth surface the voxels sample, by up to a factor
 * 1.5 for a sphere, and does not converge to it as the grid is refined.
 * There is no group form: mi_unet_group_handle(g, rank) hands out an engine to call this on. */
#define MI_UNET_VOLUME_MAX_VALUES 8
#define MI_UNET_VOLUME_MAX_TABLE 4096
typedef struct mi_unet_vcomp {      /* 88 bytes, no padding */
    int32_t voxels;                 /* voxels of the component */
    int32_t first;                  /* its raster-first voxel: z*H*W + y*W + x */
    int32_t x0, y0, z0, x1, y1, z1; /* bounding box, inclusive */
    int32_t kept;                   /* 1 when the filter keeps it, else 0 */
    int32_t value;                  /* echo of the plane's value */
    int64_t faces_x, faces_y, faces_z; /* voxel faces perpendicular to x / y / z towards a 6-neighbour that is not in the set */
    int64_t sx, sy, sz;             /* sums of x, y, z over the component */
} mi_unet_vcomp;
typedef struct mi_unet_volume_opts { int connectivity; int min_voxels; int keep_largest; } mi_unet_volume_opts; /* default { 26, 0, 0 } */
typedef struct mi_unet_vcomp_metrics { double volume_mm3, surface_mm2, cx_mm, cy_mm, cz_mm, extent_x_mm, extent_y_mm, extent_z_mm; } mi_unet_vcomp_metrics;
int mi_unet_volume_components(mi_unet_t *h, const uint8_t *masks /* [D][H][W] host */, int D, int H, int W,
                              const int *values, int n, const mi_unet_volume_opts *opts,
                              uint8_t *out /* [n][D][H][W] or NULL */, int32_t *ids /* [n][D][H][W] or NULL */,
                              mi_unet_vcomp *table /* [n][cap] */, int cap, int32_t *found /* [n] */, int32_t *kept /* [n] */);
int mi_unet_volume_components_host(const uint8_t *masks, int D, int H, int W, const int *values, int n, const mi_unet_volume_opts *opts,
                                   uint8_t *out, int32_t *ids, mi_unet_vcomp *table, int cap, int32_t *found, int32_t *kept);
int mi_unet_volume_derive(const mi_unet_vcomp *c, const double spacing_xyz[3], mi_unet_vcomp_metrics *out);

/* ---- Scores of a volume: a stack of masks against a stack of ground truth, 3-D overlap and surface distances -------
 * A stage of its own, not a setting: nothing else in this header changes behaviour because of it.  It is mi_unet_score_labels with
 * one more axis and a spacing: the same struct, the same conventions, one mi_unet_score per value.
 * Input is two byte volumes pred and truth, u8 [D][H][W] (slice z, row y, column x; D, H, W are arguments, not the engine's tile
 * size), n byte values, 1 <= n <= MI_UNET_SCORE_MAX_VALUES, and the spacing as three positive integers spacing_units = { ux, uy, uz }
 * in a unit the caller chooses (mi_unet_score_volume_units finds one for a spacing in millimetres).  Plane k compares
 * A = { pred == values[k] } with T = { truth == values[k] } over the whole volume; planes are independent.
 *   OVERLAP   tp = |A & T|, fp = |A \ T|, fn = |T \ A|, counted over all D * H * W voxels.
 *   BOUNDARY  dS = every voxel of S with a 6-neighbour that is not in S; positions outside the volume are not in S, so a set that
 *             touches a face of the volume has boundary there.  It is S & ~binary_erosion(S) with scipy's 3-D cross and
 *             border_value = 0: the surface medpy measures.  Consequence: with D = 1 every voxel of S lacks both z-neighbours, so
 *             EVERY voxel of S is a boundary voxel and n is the set size -- this is not mi_unet_score_labels on one slice.
 *   DISTANCE  between voxel centres, kept SQUARED, in integers: d2(p, q) = (dx ux)^2 + (dy uy)^2 + (dz uz)^2.  For p in dA,
 *             d2(p) = min over q in dT of d2(p, q) (direction a_to_t), and likewise from dT to dA (t_to_a).  Per direction, as in the
 *             2-D stage: n = boundary voxels of the source set, max_d2, sum_d2, sum_d_q16 = the sum of floor(2^16 sqrt(d2)), every
 *             term the exact integer floor; q_d2 = s[n - 1 - floor(n * quantile_ppm / 1000000)] of the direction's values sorted
 *             ascending, q_d2_sym the same statistic over both directions' values together.  All of it is independent of the order of
 *             evaluation and bit-reproducible.
 *   EMPTY     when dA or dT is empty both n fields still hold the counts, every max_d2, q_d2 and q_d2_sym is -1 and the sums are 0.
 * Limits, each with its reason:
 *   D, H, W in 1 .. MI_UNET_SCORE_VOLUME_MAX_SIDE = 8192: the device form keeps one row of 32-bit partial distances (4 W bytes) and
 *             the row's source list (2 W bytes) in LDS, 6 * 8192 = 48 KiB, inside the 64 KiB a launch gets without opting in;
 *   n * D * H * W < 2^31: every index and every count is an int;
 *   every unit >= 1, and ((W - 1) ux)^2 + ((H - 1) uy)^2 + ((D - 1) uz)^2 < 2^31: every d2 is a positive int32_t, so the 16 + 16-bit
 *             select of the 2-D stage applies.  A direction has fewer than 2^31 values, so sum_d2 < 2^31 * 2^31 = 2^62; every
 *             sqrt(d2) < 2^15.5 gives a term below 2^31.5 and sum_d_q16 < 2^62.5: both inside int64_t.
 * A 64 x 512 x 512 stack at 0.7 x 0.7 x 5 mm fits with a unit of 0.02 mm (35, 35, 250) and with 0.1 mm (7, 7, 50).
 * The confusion matrix (optional; opts->classes in 1 .. MI_UNET_SCORE_MAX_CLASSES, confusion and skipped not NULL) treats the volume
 * as one image: int64 [classes][classes], row = the truth byte, column = the pred byte; voxels where either byte is >= classes are
 * left out of it and counted in int64 skipped[1].
 * mi_unet_score_volume takes host buffers of any size; its workspace grows on demand, belongs to the handle (it is the one
 * mi_unet_score_labels uses) and is freed by mi_unet_destroy.  It needs the device, not the network: it works before weights are
 * loaded.  It changes no setting and nothing mi_unet_last_regions or mi_unet_last_stage_ms report.  opts == NULL is { 50000, 0 }.
 * MI_UNET_EARG with a message, nothing queued and no output written: a null pred, truth, values, spacing_units or scores; D, H or W
 * outside 1 .. 8192; n outside 1 .. MI_UNET_SCORE_MAX_VALUES; a value outside 0 .. 255 or repeated; n * D * H * W >= 2^31; a unit < 1;
 * the d2 limit; quantile_ppm outside 0 .. 999999; classes outside 0 .. 16; confusion given with classes == 0 or without skipped.
 * confusion == NULL skips the matrix whatever classes says.  A workspace that cannot be allocated is MI_UNET_EHIP with a message,
 * before anything runs; the handle stays usable.
 * mi_unet_score_volume_host is the definition as sequential host arithmetic (needs no device), same arguments without the handle,
 * same bytes.
 * mi_unet_score_volume_units is pure host arithmetic: the largest k in 0 .. 4 such that with unit_mm = 10^-k every
 * units[a] = llround(spacing_mm[a] / unit_mm) is >= 1 and the d2 limit holds for D, H, W.  The spacing actually used is
 * units[a] * unit_mm.  MI_UNET_EARG, outputs untouched: a null pointer, D, H or W outside the limits, a spacing that is not finite and
 * > 0, or no such k.
 * mi_unet_score_volume_derive is pure host arithmetic: dice, iou, precision and recall as mi_unet_score_derive gives them; hd, hd_q,
 * assd and rmsd are its values times unit_mm (NaN when the distance fields are -1).  MI_UNET_EARG for a null pointer or a unit_mm that
 * is not finite and > 0.
 * There is no group form: mi_unet_group_handle(g, rank) hands out an engine to call this on. */
#define MI_UNET_SCORE_VOLUME_MAX_SIDE 8192
int mi_unet_score_volume(mi_unet_t *h, const uint8_t *pred, const uint8_t *truth, int D, int H, int W, const int *values, int n,
                         const int spacing_units[3] /* x, y, z */, const mi_unet_score_opts *opts, mi_unet_score *scores /* [n] */,
                         int64_t *confusion /* [classes][classes] or NULL */, int64_t *skipped /* [1] */);
int mi_unet_score_volume_host(const uint8_t *pred, const uint8_t *truth, int D, int H, int W, const int *values, int n,
                              const int spacing_units[3], const mi_unet_score_opts *opts, mi_unet_score *scores, int64_t *confusion,
                              int64_t *skipped);
int mi_unet_score_volume_units(const double spacing_mm[3], int D, int H, int W, int units[3], double *unit_mm);
int mi_unet_score_volume_derive(const mi_unet_score *s, double unit_mm, mi_unet_score_metrics *out);

/* ---- Volume clean-up: 3-D cavity fill, then close and open by a ball in the caller's spacing unit -------------------
 * A stage of its own, not a setting: nothing else in this header changes behaviour because of it.  It is the 2-D tail's hole fill ->
 * close -> open (mi_unet_set_morph, 7.7) with one more axis and a spacing; the size filter behind them is mi_unet_volume_components.
 * Input is one byte volume masks, u8 [D][H][W] (slice z, row y, column x; D, H, W are arguments, not the engine's tile size), n byte
 * values, 1 <= n <= MI_UNET_VOLUME_MAX_VALUES, and the spacing as three positive integers spacing_units = { ux, uy, uz } in a unit the
 * caller chooses (mi_unet_score_volume_units finds one for a spacing in millimetres).
 *   SETS    plane k is S = { masks == values[k] }; planes are independent.  out[k] ([n][D][H][W]) is values[k] on the cleaned set and 0
 *           elsewhere (so the plane of value 0 is all zero; its stats are still exact).  out may be masks itself when n == 1.
 *   BALL    radius r in the caller's unit: B(r) = { (dx, dy, dz) : (dx ux)^2 + (dy uy)^2 + (dz uz)^2 <= r^2 }, in integer arithmetic.
 *           Its half-widths are ex = r / ux, ey = r / uy, ez = r / uz, rounded down.  r smaller than every unit is the single voxel, the
 *           identity; r between the in-plane units and uz is a flat disc; with units (1, 1, 1) its slice dz = 0 is MI_UNET_MORPH_DISC.
 *           mi_unet_volume_ball is pure host arithmetic: it writes extent = { ex, ey, ez } and, when elem is not NULL,
 *           (2 ez + 1) (2 ey + 1) (2 ex + 1) bytes 0 / 1, z-major (slice after slice, row after row).
 *   STEPS   in the order of the 2-D tail:
 *           1. if fill: add every voxel not in S that is not 6-connected, through voxels not in S, to a voxel on one of the six faces
 *              of the volume (scipy's binary_fill_holes with the 3-D cross).  With D = 1, or any side of 1, every voxel lies on a face
 *              and nothing is filled -- this is not the 2-D hole fill on one slice.  Background that reaches the outside only across
 *              an edge or a corner is a cavity and is filled.
 *           2. close: dilate by B(close_r), then erode by it.
 *           3. open: erode by B(open_r), then dilate by it.
 *   BORDER  the rules of the 2-D tail: an erosion is constrained only by voxels inside the volume, a dilation is seeded only by voxels
 *           inside the volume.  With them close is extensive, open is anti-extensive, both are idempotent, and each is the dual of the
 *           other under complement.
 *   STATS   in_voxels = |S|; filled and closed = the voxels steps 1 and 2 add; opened = the voxels step 3 removes;
 *           out_voxels = in_voxels + filled + closed - opened; value echoes values[k]; reserved is 0.  stats may be NULL.
 * Limits, each with its reason:
 *   D, H, W >= 1; n * D * H * W < 2^31: every index and every count of a plane is an int;
 *   values in 0 .. 255 and not repeated;
 *   every unit in 1 .. 46340 and both radii in 0 .. MI_UNET_VOLUME_CLEAN_MAX_R = 46340: r * r < 2^31, every offset of the ball has
 *           dx ux <= r, so every squared term is a positive int32_t and a sum of two stays inside 32 unsigned bits; an index distance
 *           along z is at most 46340 and is kept in 16 bits.  A half-width larger than the side it runs along acts as the side.
 *   The device form stages nothing per row in LDS, so there is no limit on a side beyond the product above.
 * opts == NULL is { 1, 0, 0 }: fill only.  fill is 0 or 1.
 * mi_unet_volume_clean takes host buffers of any size; its workspace (about 7 bytes per voxel and plane) grows on demand, belongs to
 * the handle and is freed by mi_unet_destroy.  It needs the device, not the network: it works before weights are loaded.  It changes
 * no setting and nothing mi_unet_last_regions or mi_unet_last_stage_ms report.  MI_UNET_EARG with a message, nothing queued and no
 * output written: a null masks, values, spacing_units or out; D, H or W < 1; n outside 1 .. MI_UNET_VOLUME_MAX_VALUES; a value outside
 * 0 .. 255 or repeated; n * D * H * W >= 2^31; a unit outside 1 .. 46340; fill other than 0 or 1; a radius outside 0 .. 46340; out ==
 * masks with n > 1.  A workspace that cannot be allocated is MI_UNET_EHIP with a message, before anything runs; the handle stays usable.
 * mi_unet_volume_clean_host is the definition as sequential host arithmetic (needs no device), same arguments without the handle,
 * same bytes.
 * mi_unet_volume_ball: MI_UNET_EARG, outputs untouched, for a null spacing_units or extent, a unit outside 1 .. 46340 or r outside
 * 0 .. 46340.
 * There is no group form: mi_unet_group_handle(g, rank) hands out an engine to call this on. */
#define MI_UNET_VOLUME_CLEAN_MAX_R 46340           /* r*r < 2^31 */
typedef struct mi_unet_volume_clean_opts { int fill; int close_r; int open_r; } mi_unet_volume_clean_opts;   /* default { 1, 0, 0 } */
typedef struct mi_unet_volume_clean_stat {         /* 48 bytes, no padding */
    int32_t value, reserved;                       /* echo of the plane's value; 0 */
    int64_t in_voxels, filled, closed, opened, out_voxels;
} mi_unet_volume_clean_stat;
int mi_unet_volume_clean(mi_unet_t *h, const uint8_t *masks /* [D][H][W] host */, int D, int H, int W, const int *values, int n,
                         const int spacing_units[3] /* x, y, z */, const mi_unet_volume_clean_opts *opts,
                         uint8_t *out /* [n][D][H][W] */, mi_unet_volume_clean_stat *stats /* [n] or NULL */);
int mi_unet_volume_clean_host(const uint8_t *masks, int D, int H, int W, const int *values, int n, const int spacing_units[3],
                              const mi_unet_volume_clean_opts *opts, uint8_t *out, mi_unet_volume_clean_stat *stats);
int mi_unet_volume_ball(const int spacing_units[3], int r, int extent[3] /* x, y, z half-widths */, uint8_t *elem /* or NULL */);

/* ---- Volume mesh: the border of a stack of masks as a closed surface of oriented quads over shared vertices ----------
 * A stage of its own, not a setting: nothing else in this header changes behaviour because of it.  It is the 3-D counterpart of the
 * contour stage: every exposed voxel face of a set becomes one quad.  Exact in integers; millimetres enter only in the two host
 * functions behind it.
 * Input is one byte volume masks, u8 [D][H][W] (slice z, row y, column x; D, H, W are arguments, not the engine's tile size), and n
 * byte values, 1 <= n <= MI_UNET_VOLUME_MAX_VALUES.  Plane k is the set S = { masks == values[k] }; positions outside the volume are
 * not in S; planes are independent.
 *   QUADS        one quad for every voxel v = (x, y, z) of S and every direction d whose 6-neighbour is not in S, the directions in the
 *                order -x, +x, -y, +y, -z, +z.  The quads of a plane are ordered by (z * H * W + y * W + x, d) ascending.  quads_x /
 *                _y / _z count them by the axis they are perpendicular to: the sums of faces_x / _y / _z over all components of the plane
 *                in mi_unet_volume_components, at any connectivity.
 *   CORNERS      grid corner (i, j, k), 0 <= i <= W, 0 <= j <= H, 0 <= k <= D, has the index c = (k * (H + 1) + j) * (W + 1) + i; voxel
 *                (x, y, z) spans the corners x .. x + 1, y .. y + 1, z .. z + 1.  A corner is a vertex of the plane iff at least one
 *                quad uses it.  Vertices are ordered by c ascending; a vertex's index is its rank.
 *   ORIENTATION  a quad lists its four vertex indices from the corner with the smallest c, then round the face counter-clockwise as
 *                seen from outside S: the right-hand normal points out of S.  Relative to (x, y, z):
 *                  -x: (0,0,0) (0,0,1) (0,1,1) (0,1,0)      +x: (1,0,0) (1,1,0) (1,1,1) (1,0,1)
 *                  -y: (0,0,0) (1,0,0) (1,0,1) (0,0,1)      +y: (0,1,0) (0,1,1) (1,1,1) (1,1,0)
 *                  -z: (0,0,0) (0,1,0) (1,1,0) (1,0,0)      +z: (0,0,1) (1,0,1) (1,1,1) (0,1,1)
 *                Wherever triangles are needed they are (0, 1, 2), (0, 2, 3).  Every directed edge is matched by its reverse, so the
 *                surface is closed; an edge where two voxels of S touch only along it is used by four quads (non-manifold).
 *   PLACEMENT    a vertex carries its corner (x, y, z) and an offset (ox, oy, oz, n); its position in voxel units is
 *                corner + o / (2 n) per axis.
 *                MI_UNET_MESH_FACES: o = 0, n = 1: the vertices sit at the voxel corners, the mesh encloses exactly |S| voxels and its
 *                  area is the crack surface of mi_unet_volume_derive.
 *                MI_UNET_MESH_NETS (naive surface nets): the eight voxel positions round the corner, (i - 1 .. i, j - 1 .. j, k - 1 .. k),
 *                  have twelve axis-parallel edges; an edge is cut when exactly one of its two ends is in S.  n = the number of cut
 *                  edges (3 .. 9 or 12; n >= 1 holds exactly for the vertices) and o = the sum over the cut edges of the edge's midpoint
 *                  in doubled units relative to the corner: 0 on the edge's own axis, -1 or +1 on the other two for the lower or higher
 *                  index.  |o| < n on every axis, so a vertex stays strictly inside the unit cube centred on its corner and no two
 *                  vertices coincide.  For a digitised ball the area is within a few per cent of the sphere's (1.030, 1.014, 1.025 of
 *                  4 pi r^2 at r = 6, 12, 20, where FACES gives 1.499, 1.462, 1.500) and the enclosed volume 0.97 .. 0.995 of |S|.
 *                Both placements have the same quads and the same vertex order.
 *   COUNTS       stats[k] is always exact, whatever the caps are: value and placement echo the arguments; quads, verts, quads_x, _y, _z.
 *   CAPS         verts[k] ([n][cap_verts]) and quads[k] ([n][cap_quads][4]) hold the first min(count, cap) entries in the orders above;
 *                the entries behind them are all zero.  A quad in the kept prefix keeps its true vertex indices even where they are
 *                >= cap_verts.  verts == NULL requires cap_verts == 0 and is legal, and so for quads: the counting call.
 * Limits, each with its reason:
 *   D, H, W >= 1;
 *   6 * (D + 1) * (H + 1) * (W + 1) < 2^31: every corner index, every quad offset of a plane and every count is an int (1024 x 512 x 512
 *           fits); planes are processed one after another, so n does not enter;
 *   values in 0 .. 255 and not repeated; placement one of the two; caps in 0 .. 2^31 - 1.
 * mi_unet_volume_mesh takes host buffers of any size; its workspace (6 bytes per voxel, the kept prefixes of one plane) grows on demand,
 * belongs to the handle and is freed by mi_unet_destroy.  It needs the device, not the network: it works before weights are loaded.  It
 * changes no setting and nothing mi_unet_last_regions or mi_unet_last_stage_ms report.  MI_UNET_EARG with a message, nothing queued and
 * nothing written: a null masks, values or stats; D, H or W < 1; n outside 1 .. MI_UNET_VOLUME_MAX_VALUES; a value outside 0 .. 255 or
 * repeated; the corner limit; a placement other than the two; a negative cap; a NULL array with a cap other than 0.  A workspace that
 * cannot be allocated is MI_UNET_EHIP with a message; the handle stays usable.
 * mi_unet_volume_mesh_host is the definition as sequential host arithmetic (needs no device), same arguments without the handle, same
 * bytes.
 * mi_unet_volume_mesh_positions and mi_unet_volume_mesh_derive are pure host arithmetic in double.  A voxel is a box of
 * spacing_xyz[0] x [1] x [2] millimetres and corner 0 is at 0: a vertex lies at (corner + o / (2.0 * n)) * spacing per axis, which
 * _positions rounds once to float.  _derive walks the quads in order and their two triangles (a, b, c) in order and accumulates
 * area_mm2 += 0.5 |(b - a) x (c - a)| and volume_mm3 += a . (b x c) / 6 sequentially; the volume is positive for the outward
 * orientation above.  nq quads refer to nv vertices.  MI_UNET_EARG, outputs untouched: a null pointer (quads may be NULL when nq == 0,
 * verts and xyz when nv == 0); nv or nq < 0; n == 0 in a vertex; an index outside 0 .. nv - 1; a spacing that is not finite and > 0.
 * There is no group form: mi_unet_group_handle(g, rank) hands out an engine to call this on. */
#define MI_UNET_MESH_FACES 0
#define MI_UNET_MESH_NETS  1
typedef struct mi_unet_mesh_vertex {               /* 16 bytes, no padding */
    int32_t x, y, z;                               /* the grid corner */
    int8_t ox, oy, oz;                             /* offset in units of 1 / (2 n) voxel */
    uint8_t n;                                     /* cut edges round the corner (NETS), or 1 (FACES) */
} mi_unet_mesh_vertex;
typedef struct mi_unet_mesh_stat {                 /* 48 bytes, no padding */
    int32_t value, placement;                      /* echo of the plane's value and of the placement */
    int64_t quads, verts, quads_x, quads_y, quads_z;
} mi_unet_mesh_stat;
typedef struct mi_unet_mesh_metrics { double area_mm2, volume_mm3; } mi_unet_mesh_metrics;
int mi_unet_volume_mesh(mi_unet_t *h, const uint8_t *masks /* [D][H][W] host */, int D, int H, int W, const int *values, int n,
                        int placement, mi_unet_mesh_vertex *verts /* [n][cap_verts] or NULL */, int cap_verts,
                        int32_t *quads /* [n][cap_quads][4] or NULL */, int cap_quads, mi_unet_mesh_stat *stats /* [n] */);
int mi_unet_volume_mesh_host(const uint8_t *masks, int D, int H, int W, const int *values, int n, int placement,
                             mi_unet_mesh_vertex *verts, int cap_verts, int32_t *quads, int cap_quads, mi_unet_mesh_stat *stats);
int mi_unet_volume_mesh_positions(const mi_unet_mesh_vertex *verts, int nv, const double spacing_xyz[3], float *xyz /* [nv][3] */);
int mi_unet_volume_mesh_derive(const mi_unet_mesh_vertex *verts, int nv, const int32_t *quads /* [nq][4] */, int nq,
                               const double spacing_xyz[3], mi_unet_mesh_metrics *out);

/* ---- Volume measurement: per component of a labelled stack its moments, its intensity and its longest diameters ------
 * A stage of its own, not a setting: nothing else in this header changes behaviour because of it.  It is mi_unet_region (7.6) with one
 * more axis, plus the longest diameter in 3-D and within one slice (the RECIST long axis).  Exact in integers; millimetres enter only
 * in mi_unet_volume_measure_derive.
 * Input is ids, int32 [D][H][W] (slice z, row y, column x; D, H, W are arguments, not the engine's tile size), optionally intensity,
 * uint16 [D][H][W], the number of components m and the spacing as three positive integers spacing_units = { ux, uy, uz } in a unit the
 * caller chooses (mi_unet_score_volume_units finds one for a spacing in millimetres).
 *   COMPONENT  component r, 0 <= r < m, is the set of voxels with ids == r + 1: exactly what mi_unet_volume_components writes into ids.
 *              Every other value (0, -1, anything above m) belongs to no component.  The stage does not ask whether a set is connected.
 *              A voxel's index is z * H * W + y * W + x.  An id that no voxel carries gives an all-zero entry.
 *   SUMS       voxels, sx, sy, sz and sxx, syy, szz, sxy, sxz, syz are taken over the component's integer coordinates; si, sii (the sums
 *              of v and v * v), imin and imax over intensity.  The four are 0 when intensity is NULL.
 *   RUN ENDS   a voxel of the component is a run end when its x - 1 or its x + 1 neighbour on the same row is not in the component;
 *              positions outside the volume are not in it.  ends is their count and is always exact.
 *   DIAMETER   with d2(p, q) = (dx ux)^2 + (dy uy)^2 + (dz uz)^2 between voxel centres (the distance of mi_unet_score_volume), d2 is the
 *              maximum over all pairs of voxels of the component, p == q included.  Among the pairs (p <= q by index) that reach the
 *              maximum, dp, dq are the one with the smallest p, then the smallest q.  One voxel gives 0 with p = q.  a_d2, a_p, a_q
 *              follow the same rule over the pairs with equal z.
 *              The result is defined over all voxels, but only run ends can take part in a maximal pair: squared distance is strictly
 *              convex, so a voxel strictly between two others of the component on a line is strictly nearer to any q than one of the
 *              two is (DESIGN.md 7.13 has the proof).  Both forms search the run ends only.
 *   CAP        the search costs ends^2 per component.  A component with ends > max_ends, and every component when max_ends == 0, gets
 *              -1 in all six diameter fields; everything else in its entry stays valid (an id that no voxel carries is no component: its
 *              entry stays all-zero).  The cap acts on ends, a defined quantity, so the two forms agree on who is skipped.
 * Limits, each with its reason:
 *   D, H, W in 1 .. MI_UNET_SCORE_VOLUME_MAX_SIDE: a coordinate is below 2^13, so sxx < 2^31 * 2^26 = 2^57;
 *   D * H * W < 2^31: every index and every count is an int;
 *   m in 1 .. MI_UNET_VOLUME_MAX_TABLE: what mi_unet_volume_components can have numbered;
 *   every unit >= 1, and ((W - 1) ux)^2 + ((H - 1) uy)^2 + ((D - 1) uz)^2 < 2^31 (the limit of mi_unet_score_volume): every d2 is an
 *           int32_t and a pre-scaled coordinate an int;
 *   max_ends in 0 .. MI_UNET_VMEASURE_MAX_ENDS_LIMIT = 2^20: 2^40 pairs, the most one component may cost;
 *   sii < 2^31 * 65535^2 < 2^63: inside int64_t.
 * opts == NULL is { 262144 }.
 * mi_unet_volume_measure takes host buffers of any size; its workspace grows on demand, belongs to the handle and is freed by
 * mi_unet_destroy.  It needs the device, not the network: it works before weights are loaded.  It changes no setting and nothing
 * mi_unet_last_regions or mi_unet_last_stage_ms report.  MI_UNET_EARG with a message, nothing queued and no output written: a null ids,
 * spacing_units or table; D, H or W outside 1 .. 8192; D * H * W >= 2^31; m outside 1 .. MI_UNET_VOLUME_MAX_TABLE; a unit < 1; the d2
 * limit; max_ends outside 0 .. 2^20.  A workspace that cannot be allocated is MI_UNET_EHIP with a message; the handle stays usable.
 * mi_unet_volume_measure_host is the definition as sequential host arithmetic (needs no device), same arguments without the handle,
 * same bytes.
 * mi_unet_volume_measure_derive is pure host arithmetic in double.  A voxel is a box of s = spacing_units * unit_mm millimetres per axis
 * and voxel 0 spans 0 .. 1 of the grid.  With A = voxels:
 *   c*_mm = (sum / A + 0.5) * s of the axis, as mi_unet_volume_derive gives it.
 *   The central second moments have exact 128-bit integer numerators that are converted once (as mi_unet_region_derive):
 *   C_ab = (A * s_ab - s_a * s_b) / A^2 * s[a] * s[b], in mm^2, and every diagonal gains s[a]^2 / 12 because a voxel is a box.
 *   The eigenvalues of C come from a cyclic Jacobi solver with a fixed number of sweeps (16; no library), descending:
 *   axis_mm[i] = 2 sqrt(5 lambda_i), the full axes of the solid ellipsoid with these moments (one voxel gives 1.291 s per axis);
 *   axis_dir[i] is the unit eigenvector (x, y, z), its sign chosen so that its component of largest magnitude is positive.
 *   mean = si / A and std = sqrt((A * sii - si^2) / A^2).
 *   diameter_mm = sqrt(d2) * unit_mm and axial_diameter_mm = sqrt(a_d2) * unit_mm; NaN when the field is -1.
 * MI_UNET_EARG, output untouched: a null pointer, voxels < 1, a unit < 1, or a unit_mm that is not finite and > 0.
 * There is no group form: mi_unet_group_handle(g, rank) hands out an engine to call this on. */
#define MI_UNET_VMEASURE_MAX_ENDS_LIMIT 1048576   /* 2^20 */
typedef struct mi_unet_vmeasure {      /* 128 bytes, no padding */
    int32_t voxels, ends;              /* voxels with this id; its run ends */
    int32_t imin, imax;                /* min / max of intensity over the component; 0, 0 without intensity */
    int32_t d2, dp, dq;                /* longest diameter: squared, in units^2, and the voxel indices of its ends */
    int32_t a_d2, a_p, a_q;            /* the same restricted to pairs in one slice (dz == 0) */
    int64_t sx, sy, sz;                /* sums of x, y, z over the component */
    int64_t sxx, syy, szz, sxy, sxz, syz;
    int64_t si, sii;                   /* sum v, sum v*v of the intensity */
} mi_unet_vmeasure;
typedef struct mi_unet_vmeasure_opts { int max_ends; } mi_unet_vmeasure_opts;     /* default { 262144 } */
typedef struct mi_unet_vmeasure_shape { double cx_mm, cy_mm, cz_mm, axis_mm[3], axis_dir[3][3], mean, std, diameter_mm, axial_diameter_mm; } mi_unet_vmeasure_shape;
int mi_unet_volume_measure(mi_unet_t *h, const int32_t *ids /* [D][H][W] host */, const uint16_t *intensity /* [D][H][W] host or NULL */,
                           int D, int H, int W, int m, const int spacing_units[3], const mi_unet_vmeasure_opts *opts,
                           mi_unet_vmeasure *table /* [m] */);
int mi_unet_volume_measure_host(const int32_t *ids, const uint16_t *intensity, int D, int H, int W, int m, const int spacing_units[3],
                                const mi_unet_vmeasure_opts *opts, mi_unet_vmeasure *table);
int mi_unet_volume_measure_derive(const mi_unet_vmeasure *c, const int spacing_units[3], double unit_mm, mi_unet_vmeasure_shape *out);

/* ---- Volume matching: the components of a prediction against the components of a truth, lesion by lesion ----------------
 * A stage of its own, not a setting: nothing else in this header changes behaviour because of it.  Everything up to
 * mi_unet_volume_match_derive is an exact integer and independent of the order of evaluation.
 * Input is pred_ids and truth_ids, both int32 [D][H][W] (slice z, row y, column x; D, H, W are arguments, not the engine's tile size),
 * and the component counts mp and mt.
 *   COMPONENT  pred component r, 0 <= r < mp, is the set of voxels with pred_ids == r + 1: exactly what mi_unet_volume_components writes
 *              into ids.  Truth component c, 0 <= c < mt, likewise.  Every other value (0, -1, anything above the side's m) is class 0,
 *              "no component".  The stage does not ask whether a set is connected.
 *   TABLE      N[a][b], 0 <= a <= mp, 0 <= b <= mt, is the number of voxels whose pred class is a and whose truth class is b; a class is
 *              0 or index + 1.  N[0][0] is not reported.
 *   SIDES      one entry per pred component r, and the mirror image (rows and columns exchanged) per truth component:
 *                voxels       sum over b of N[r + 1][b];
 *                covered      voxels - N[r + 1][0]: its voxels that lie in any component of the other side;
 *                partners     the number of b >= 1 with N[r + 1][b] > 0;
 *                best         1 + the index of the partner with the largest intersection, ties to the smallest index; 0 when there is none;
 *                best_voxels  that intersection (0 when there is none).
 *              They are always exact, whatever cap is.  An id that no voxel carries gives an all-zero entry.
 *   PAIRS      *found is the number of (a >= 1, b >= 1) with N[a][b] > 0; it is always exact.  pairs [cap] holds the first
 *              min(found, cap) of them as { p, t, voxels } with p = a - 1 and t = b - 1, ordered by p ascending, then t ascending; the
 *              entries behind them are all-zero.
 * Limits, each with its reason:
 *   D, H, W >= 1;
 *   D * H * W < 2^31: every count is an int32_t;
 *   mp, mt in 1 .. MI_UNET_VOLUME_MAX_TABLE: what mi_unet_volume_components can have numbered; the table has at most 4097^2 cells (67 MB);
 *   cap >= 1.
 * mi_unet_volume_match takes host buffers of any size; its workspace (both stacks, the dense table, the results) grows on demand,
 * belongs to the handle and is freed by mi_unet_destroy.  It needs the device, not the network: it works before weights are loaded.
 * It changes no setting and nothing mi_unet_last_regions or mi_unet_last_stage_ms report.  MI_UNET_EARG with a message, nothing queued
 * and no output written: a null pointer, or any limit broken.  A workspace that cannot be allocated is MI_UNET_EHIP with a message; the
 * handle stays usable.
 * mi_unet_volume_match_host is the definition as sequential host arithmetic (needs no device), same arguments without the handle, same
 * bytes.
 * mi_unet_volume_match_assign is pure host arithmetic: a one-to-one assignment at an IoU threshold iou_num / iou_den,
 * 1 <= iou_num <= iou_den <= 65536.  With i a pair's voxels, vp and vt the voxels of its two components, the union is u = vp + vt - i.
 *   A pair is a candidate iff i * iou_den >= iou_num * u, compared in 64-bit integers.
 *   Candidates are ordered by IoU descending: i1 * u2 against i2 * u1, both below 2^63, so the comparison is exact.  Ties go by p
 *   ascending, then t ascending, so the order is total.  Walking that order, a candidate is accepted iff neither of its components is
 *   taken yet.
 *   match_of_pred [mp] and match_of_truth [mt] hold 1 + the partner, or 0.  counts = { tp, fp, fn } with tp the accepted pairs,
 *   fp = mp_present - tp and fn = mt_present - tp; a component is present when its voxels > 0.
 *   Above a threshold of 1/2 the candidates are already one-to-one (two candidates that share a component would each hold more than half
 *   of it, and they are disjoint), so every assignment rule gives this result.  At or below 1/2 the assignment is greedy, not the optimal
 *   one.
 *   MI_UNET_EARG, output untouched: a null pointer, mp or mt outside 1 .. MI_UNET_VOLUME_MAX_TABLE, cap < 1, found < 0, a truncated
 *   pair list (found > cap), a threshold outside its range, or a pair that names a component outside the tables.
 * mi_unet_volume_match_derive is pure host arithmetic in double over the matches in pred order, so every sum has one value.  With
 * IoU = i / u and Dice = 2 i / (vp + vt) of a match:
 *   precision = tp / (tp + fp), recall = tp / (tp + fn), f1 = 2 tp / (2 tp + fp + fn);
 *   sq = sum IoU / tp, rq = tp / (tp + fp / 2 + fn / 2), pq = sq * rq (panoptic quality); mean_dice = sum Dice / tp.
 *   A quantity is NaN where its denominator is 0.  tp, fp, fn are recounted from match_of_pred and the side tables.
 *   MI_UNET_EARG, output untouched: a null pointer, a size outside its range, found > cap, or a match that is not in the pair list.
 * There is no group form: mi_unet_group_handle(g, rank) hands out an engine to call this on. */
typedef struct mi_unet_vmatch_side { int32_t voxels, covered, partners, best, best_voxels; } mi_unet_vmatch_side;   /* 20 bytes */
typedef struct mi_unet_vmatch_pair { int32_t p, t, voxels; } mi_unet_vmatch_pair;                                   /* 12 bytes */
typedef struct mi_unet_vmatch_counts { int32_t tp, fp, fn; } mi_unet_vmatch_counts;
typedef struct mi_unet_vmatch_scores { double precision, recall, f1, sq, rq, pq, mean_dice; } mi_unet_vmatch_scores;
int mi_unet_volume_match(mi_unet_t *h, const int32_t *pred_ids /* [D][H][W] host */, const int32_t *truth_ids /* [D][H][W] host */,
                         int D, int H, int W, int mp, int mt, int cap, mi_unet_vmatch_side *pred_side /* [mp] */,
                         mi_unet_vmatch_side *truth_side /* [mt] */, mi_unet_vmatch_pair *pairs /* [cap] */, int *found);
int mi_unet_volume_match_host(const int32_t *pred_ids, const int32_t *truth_ids, int D, int H, int W, int mp, int mt, int cap,
                              mi_unet_vmatch_side *pred_side, mi_unet_vmatch_side *truth_side, mi_unet_vmatch_pair *pairs, int *found);
int mi_unet_volume_match_assign(const mi_unet_vmatch_side *pred_side, int mp, const mi_unet_vmatch_side *truth_side, int mt,
                                const mi_unet_vmatch_pair *pairs, int found, int cap, int iou_num, int iou_den,
                                int32_t *match_of_pred /* [mp] */, int32_t *match_of_truth /* [mt] */, mi_unet_vmatch_counts *counts);
int mi_unet_volume_match_derive(const mi_unet_vmatch_side *pred_side, int mp, const mi_unet_vmatch_side *truth_side, int mt,
                                const mi_unet_vmatch_pair *pairs, int found, int cap, const int32_t *match_of_pred /* [mp] */,
                                mi_unet_vmatch_scores *out);

/* ---- Volume texture: per component of a labelled stack its grey-level histogram and its 3-D co-occurrence tables ----------
 * A stage of its own, not a setting: nothing else in this header changes behaviour because of it.  Everything up to
 * mi_unet_volume_texture_derive is an exact integer count and independent of the order of evaluation.
 * Input is ids, int32 [D][H][W] (slice z, row y, column x; D, H, W are arguments, not the engine's tile size), intensity, uint16
 * [D][H][W], and the number of components m; both buffers are required.
 *   COMPONENT  as in mi_unet_volume_measure: component r, 0 <= r < m, is the set of voxels with ids == r + 1.  Every other value (0, -1,
 *              anything above m) belongs to no component.  The stage does not ask whether a set is connected.  An id that no voxel
 *              carries gives an all-zero entry and all-zero rows.
 *   OPTIONS    opts = { mode, levels L, lo, width }; NULL is { MI_UNET_VTEX_COUNT, 32, 0, 1 }.  lo and width are read in
 *              MI_UNET_VTEX_WIDTH only, and checked in both modes.
 *   LEVEL      of a voxel of component r with value v, in integer arithmetic only:
 *              MI_UNET_VTEX_COUNT (a fixed number of bins over the component's own range): with imin, imax over the component,
 *                level = ((v - imin) * L) / (imax - imin + 1).  It is always below L; a constant component is all level 0.
 *              MI_UNET_VTEX_WIDTH (a fixed bin size, one scale for all components): level = v < lo ? 0 : min(L - 1, (v - lo) / width).
 *   TABLE      voxels; imin, imax over the component (in both modes); levels_used, the number of non-empty histogram bins; pairs and
 *              pairs_axial, the sums of the two co-occurrence tables (0 for a table that was not asked for).
 *   HIST       hist[r][l] is the number of voxels of r at level l.
 *   GLCM       the 13 offsets d = (dx, dy, dz) are the lexicographically positive half of the 26-neighbourhood: dz = 1 with any dx, dy in
 *              -1 .. 1, or dz = 0 and dy = 1 with any dx, or (1, 0, 0).  glcm[r][i][j] counts the ordered pairs (p, p + d) over those 13
 *              offsets with both voxels inside the volume, both in component r, level(p) = i and level(p + d) = j.  glcm_axial counts
 *              the same over the 4 offsets with dz = 0: the in-plane table a thick-slice series wants.  Either pointer may be NULL: that
 *              table is not computed.  The tables are not symmetrised; mi_unet_volume_texture_derive does that (P = G + G^T), so the
 *              counts stay the plain counts.
 * Limits, each with its reason:
 *   D, H, W in 1 .. MI_UNET_SCORE_VOLUME_MAX_SIDE (8192);
 *   D * H * W <= 2^28: a voxel starts at most 13 pairs, so every cell is below 13 * 2^28 < 2^32 and is a uint32_t;
 *   L in 2 .. MI_UNET_VTEX_MAX_LEVELS (64): a level and a component's number share one 32-bit key, and an L x L table fits a workgroup's LDS;
 *   m in 1 .. MI_UNET_VOLUME_MAX_TABLE and m * L * L <= MI_UNET_VTEX_MAX_CELLS (2^22): 4096 components at 32 levels, 1024 at 64; a table
 *           is at most 16 MiB;
 *   width in 1 .. 65536 and lo in 0 .. 65535: the range of a uint16_t.
 * mi_unet_volume_texture takes host buffers of any size; its workspace grows on demand, belongs to the handle and is freed by
 * mi_unet_destroy.  It needs the device, not the network: it works before weights are loaded.  It changes no setting and nothing
 * mi_unet_last_regions or mi_unet_last_stage_ms report.  MI_UNET_EARG with a message that begins "mi_unet_volume_texture:", nothing
 * queued and no output written: a null ids, intensity, table or hist; any limit broken; a mode that does not exist.  A workspace that
 * cannot be allocated is MI_UNET_EHIP with a message; the handle stays usable.
 * mi_unet_volume_texture_host is the definition as sequential host arithmetic (needs no device), same arguments without the handle,
 * same bytes.
 * mi_unet_volume_texture_derive is pure host arithmetic in double over one component's entry, its histogram row and one of its tables, with
 * a fixed summation order (i ascending, then j ascending).  Levels are numbered 1 .. L in the formulas, as the IBSI numbers them.
 *   From hist, with p_l = hist[l] / voxels and mu = sum l p_l:
 *     mean = mu; variance = sum p_l (l - mu)^2; skewness = sum p_l (l - mu)^3 / variance^1.5 and kurtosis = sum p_l (l - mu)^4 /
 *     variance^2 - 3 (the excess), both 0 when the variance is 0; median, p10 and p90 are the smallest level whose cumulative count reaches
 *     ceil(q * voxels) for q = 1/2, 1/10, 9/10, in exact integers; mode is the fullest level, ties to the smallest; entropy = - sum p_l
 *     log2 p_l; uniformity = sum p_l^2.
 *   From one table G with its sum `pairs` (c->pairs for glcm, c->pairs_axial for glcm_axial: the function adds G up itself), with
 *   p_ij = (G_ij + G_ji) / (2 pairs) and mu = sum i p_ij:
 *     joint_max = max p_ij; joint_average = mu; joint_variance = sum (i - mu)^2 p_ij; joint_entropy = - sum p_ij log2 p_ij;
 *     contrast = sum (i - j)^2 p_ij; dissimilarity = sum |i - j| p_ij; inverse_difference = sum p_ij / (1 + |i - j|);
 *     inverse_difference_moment = sum p_ij / (1 + (i - j)^2); angular_second_moment = sum p_ij^2;
 *     correlation = sum (i - mu)(j - mu) p_ij / joint_variance.
 *   Every one of the ten is NaN when glcm is NULL or the table's sum is 0; correlation is NaN when joint_variance is 0.
 * MI_UNET_EARG, output untouched: a null c, hist or out; voxels < 1; L outside 2 .. 64.
 * There is no group form: mi_unet_group_handle(g, rank) hands out an engine to call this on. */
#define MI_UNET_VTEX_COUNT 0
#define MI_UNET_VTEX_WIDTH 1
#define MI_UNET_VTEX_MAX_LEVELS 64
#define MI_UNET_VTEX_MAX_CELLS 4194304          /* 2^22 */
#define MI_UNET_VTEX_MAX_VOXELS 268435456       /* 2^28 */
typedef struct mi_unet_vtexture_opts { int mode, levels, lo, width; } mi_unet_vtexture_opts;    /* default { MI_UNET_VTEX_COUNT, 32, 0, 1 } */
typedef struct mi_unet_vtexture {      /* 32 bytes, no padding */
    int32_t voxels, imin, imax;        /* voxels with this id; min / max of intensity over them */
    int32_t levels_used;               /* non-empty histogram bins */
    int64_t pairs, pairs_axial;        /* sums of glcm[r] and of glcm_axial[r]; 0 for a table that was not asked for */
} mi_unet_vtexture;
typedef struct mi_unet_vtexture_features {     /* 144 bytes, no padding */
    double mean, variance, skewness, kurtosis, entropy, uniformity;
    int32_t median, p10, p90, mode;    /* levels 1 .. L */
    double joint_max, joint_average, joint_variance, joint_entropy, contrast, dissimilarity, inverse_difference,
           inverse_difference_moment, angular_second_moment, correlation;
} mi_unet_vtexture_features;
int mi_unet_volume_texture(mi_unet_t *h, const int32_t *ids /* [D][H][W] host */, const uint16_t *intensity /* [D][H][W] host */, int D,
                           int H, int W, int m, const mi_unet_vtexture_opts *opts, mi_unet_vtexture *table /* [m] */,
                           uint32_t *hist /* [m][L] */, uint32_t *glcm /* [m][L][L] or NULL */, uint32_t *glcm_axial /* [m][L][L] or NULL */);
int mi_unet_volume_texture_host(const int32_t *ids, const uint16_t *intensity, int D, int H, int W, int m, const mi_unet_vtexture_opts *opts,
                                mi_unet_vtexture *table, uint32_t *hist, uint32_t *glcm, uint32_t *glcm_axial);
int mi_unet_volume_texture_derive(const mi_unet_vtexture *c, const uint32_t *hist /* [L] */, const uint32_t *glcm /* [L][L] or NULL */, int L,
                                  mi_unet_vtexture_features *out);

/* ---- Volume interpolation: slices put between the slices of a stack of masks, shape-based (Raya and Udupa) ------------
 * A stage of its own, not a setting: nothing else in this header changes behaviour because of it.  A thick-slice stack is a pile of
 * slabs; this stage fills the gaps with slices whose outline moves linearly from one slice's outline to the next one's.  The signed
 * in-plane distance of every slice is interpolated linearly between neighbouring slices and cut at zero -- in integers only: comparing
 * two weighted distances is comparing their weighted squares, so no square root is taken and device, host form and reference agree
 * byte for byte.
 * Input is one byte volume masks, u8 [D][H][W] (slice z, row y, column x; D, H, W are arguments, not the engine's tile size), n byte
 * values, 1 <= n <= MI_UNET_VOLUME_MAX_VALUES, the in-plane spacing as two positive integers units_xy = { ux, uy } in a unit the caller
 * chooses (the first two of mi_unet_score_volume_units), and the factor k, 1 .. MI_UNET_VINTERP_MAX_FACTOR.  The units are divided by
 * their greatest common divisor first: (7, 7) is (1, 1).  The spacing along z does not enter: the new slices divide every gap evenly.
 *   SIZES     D' = (D - 1) k + 1 output slices.  mi_unet_volume_interp_slices(D, k) returns D', or -1 for a D outside 1 .. 8192 or a k
 *             outside 1 .. 16; it is pure host arithmetic.
 *   SETS      plane v is S_z = { masks[z] == values[v] } per slice z; planes are independent.
 *   DISTANCE  for a pixel p of slice z, e_z(p) = the minimum of (ux (px - qx))^2 + (uy (py - qy))^2 over the pixels q OF THE SAME SLICE
 *             whose state (in S_z or not) differs from p's.  Positions outside the image are no candidates.  e_z(p) = NONE =
 *             MI_UNET_VINTERP_NONE = 2^31 - 1 when the slice has no such q: it is all set or all unset.
 *   SLICES    output slice i k + j, 0 <= i < D - 1, 0 <= j < k, lies between the input slices i and i + 1; output slice D' - 1 is
 *             S_{D-1}.  For j = 0 it is S_i.  For j >= 1 the weights are w_i = k - j and w_{i+1} = j, and a pixel p
 *               set in both neighbouring slices is set; set in neither is unset;
 *               set in exactly one of them (a MIXED voxel) is set iff  w_set^2 e_set(p) >= w_unset^2 e_unset(p)  in 64-bit integers,
 *               where `set` is the neighbour that holds p and `unset` the other; equality (a TIE) is set.
 *             This is the sign of (k - j) phi_i + j phi_{i+1} with phi = +sqrt(e) inside and -sqrt(e) outside, zero counted as inside.
 *             The rule is symmetric under a flip of z.  NONE takes part as the number it is: between an all-set and an all-unset
 *             slice the nearer one wins and the middle is set.
 *   OUTPUT    out u8 [n][D'][H][W]: values[v] on the set and 0 elsewhere (so the plane of value 0 is all zero; its stats are still
 *             exact).  out must not overlap masks.
 *   INTENSITY optional: intensity u16 [D][H][W] -> intensity_out u16 [D'][H][W]; slice i k + j is ((k - j) a + j b + k / 2) / k in
 *             integers, a and b the samples of slices i and i + 1; slice D' - 1 is slice D - 1.  Both pointers NULL or both not.
 *   STATS     per value: in_voxels = the voxels of S over the D input slices, out_voxels = those set in out, mixed = the mixed voxels
 *             over all new slices (j >= 1), mixed_set = those of them that are set, ties = those of them decided by equality.
 *             stats may be NULL.
 * Limits, each with its reason:
 *   D, H, W in 1 .. MI_UNET_SCORE_VOLUME_MAX_SIDE (8192): a column distance is kept in 15 bits, a row is staged in a workgroup's LDS;
 *   n * D' * H * W < 2^31: every index of out is an int;
 *   values in 0 .. 255 and not repeated; both units at least 1;
 *   ((W - 1) ux)^2 + ((H - 1) uy)^2 < 2^31 - 1 with the reduced units: every e is an int32_t below NONE; w^2 e < 2^39.
 * mi_unet_volume_interp takes host buffers of any size; its workspace (6 bytes per input voxel and plane, the stacks themselves
 * beside it) grows on demand, belongs to the handle and is freed by mi_unet_destroy.  It needs the device, not the network: it works
 * before weights are loaded.  It changes no setting and nothing mi_unet_last_regions or mi_unet_last_stage_ms report.  MI_UNET_EARG
 * with a message that begins "mi_unet_volume_interp:", nothing queued and no output written: a null masks, values, units_xy or out; one
 * of intensity and intensity_out null and the other not; any limit broken; out overlapping masks.  A workspace that cannot be
 * allocated is MI_UNET_EHIP with a message; the handle stays usable.
 * mi_unet_volume_interp_host is the definition as sequential host arithmetic (needs no device), same arguments without the handle,
 * same bytes.
 * There is no group form: mi_unet_group_handle(g, rank) hands out an engine to call this on. */
#define MI_UNET_VINTERP_MAX_FACTOR 16
#define MI_UNET_VINTERP_NONE 2147483647            /* 2^31 - 1 */
typedef struct mi_unet_vinterp_stat {              /* 40 bytes, no padding */
    int64_t in_voxels, out_voxels, mixed, mixed_set, ties;
} mi_unet_vinterp_stat;
int mi_unet_volume_interp(mi_unet_t *h, const uint8_t *masks /* [D][H][W] host */, int D, int H, int W, const int *values, int n,
                          const int units_xy[2] /* x, y */, int factor, const uint16_t *intensity /* [D][H][W] or NULL */,
                          uint8_t *out /* [n][D'][H][W] */, uint16_t *intensity_out /* [D'][H][W] or NULL */,
                          mi_unet_vinterp_stat *stats /* [n] or NULL */);
int mi_unet_volume_interp_host(const uint8_t *masks, int D, int H, int W, const int *values, int n, const int units_xy[2], int factor,
                               const uint16_t *intensity, uint8_t *out, uint16_t *intensity_out, mi_unet_vinterp_stat *stats);
int mi_unet_volume_interp_slices(int D, int factor);

/* ---- Volume zones: per component of a labelled stack its grey-level run-length and size-zone matrices -------------------
 * A stage of its own, not a setting: nothing else in this header changes behaviour because of it.  Everything up to the two feature
 * functions is an exact integer count and independent of the order of evaluation.
 * Input is ids, int32 [D][H][W], intensity, uint16 [D][H][W], and the number of components m, as mi_unet_volume_texture takes them; both
 * buffers are required.
 *   COMPONENT  exactly as in mi_unet_volume_texture: component r, 0 <= r < m, is the set of voxels with ids == r + 1.  0, -1 and anything
 *              above m belong to no component.  The stage does not ask whether a set is connected.  An id that no voxel carries gives
 *              an all-zero entry and all-zero rows.
 *   OPTIONS    opts = { mode, levels L, lo, width, max_run R }; NULL is { MI_UNET_VTEX_COUNT, 32, 0, 1, 32 }.
 *   LEVEL      mode, L, lo and width mean what they mean in mi_unet_vtexture_opts, and the level of a voxel is mi_unet_volume_texture's
 *              formula: the same stack at the same options has the same levels in both stages.  A voxel's KEY is (r + 1) << 8 | level,
 *              0 for a voxel of no component.
 *   RUNS       the 13 offsets d are mi_unet_volume_texture's, the lexicographically positive half of the 26-neighbourhood.  For an offset
 *              d a run is a maximal sequence p, p + d, .., p + (n - 1) d inside the volume whose voxels have one key that is not 0: one
 *              component r and one level l.  rlm[r][l][min(n, R) - 1] counts the runs over all 13 offsets, rlm_axial the same over the 4
 *              offsets with dz = 0.  The last bin collects every run of length >= R; the entry's `clamped` says how many runs were
 *              longer than R, so 0 there means the table is the unclamped matrix.  R = 8192 never clamps: no run is longer than the
 *              longest side.  Either pointer may be NULL: that table is not computed and its sums in the entry are 0.
 *   ZONES      a zone is a 26-connected set of voxels with one key that is not 0.  Two components that touch at one level do not merge;
 *              two separated parts of one id at one level are two zones.  *found is the number of zones over all components, always
 *              exact.  zones[cap] holds the first min(found, cap) zones as { first, component, level, size }: `first` is the linear
 *              index (z H + y) W + x of the zone's first voxel in raster order, `level` counts from 0, and the order is `first`
 *              ascending, which is total.  The entries behind them are all-zero (the rule of mi_unet_volume_match's pair list).  With
 *              zones NULL the zone half is not computed, found must be NULL too, and the entry's zone fields are 0.
 *   ENTRY      voxels, imin, imax as in mi_unet_vtexture; longest_run over the 13 offsets, unclamped (0 without rlm); zones and
 *              largest_zone, exact whatever cap is; runs and runs_axial, the two tables' sums; clamped and clamped_axial, the runs of
 *              length >= R + 1 in each.
 * Limits, each with its reason:
 *   D, H, W in 1 .. MI_UNET_SCORE_VOLUME_MAX_SIDE (8192);
 *   D * H * W <= 2^28: a voxel starts at most 13 runs, so every cell is below 13 * 2^28 < 2^32 and is a uint32_t; an index is an int32_t;
 *   L in 2 .. MI_UNET_VTEX_MAX_LEVELS (64): the key's 8 level bits, and mi_unet_volume_texture's limit;
 *   R in 2 .. MI_UNET_VZONES_MAX_RUN (8192): the longest side;
 *   m in 1 .. MI_UNET_VOLUME_MAX_TABLE and m * L * R <= MI_UNET_VTEX_MAX_CELLS (2^22): 4096 components at 32 x 32; a table is at most
 *           16 MiB;
 *   cap in 1 .. MI_UNET_VZONES_MAX_CAP (2^24) when zones is given: the list is at most 256 MiB;
 *   width in 1 .. 65536 and lo in 0 .. 65535: the range of a uint16_t; a mode that exists.
 * mi_unet_volume_zones takes host buffers of any size; its workspace grows on demand, belongs to the handle and is freed by
 * mi_unet_destroy.  It needs the device, not the network: it works before weights are loaded.  It changes no setting and nothing
 * mi_unet_last_regions or mi_unet_last_stage_ms report.  MI_UNET_EARG with a message that begins "mi_unet_volume_zones:", nothing queued
 * and no output written: a null ids, intensity or table; exactly one of zones and found NULL; any limit broken.  A workspace that
 * cannot be allocated is MI_UNET_EHIP with a message; the handle stays usable.
 * mi_unet_volume_zones_host is the definition as sequential host arithmetic (needs no device), same arguments without the handle, same
 * bytes.
 * The two feature functions are pure host arithmetic in double over the non-zero cells (i, j, count) of one component's matrix: i =
 * level + 1 (the IBSI's numbering), j = the run length (bin + 1) or the zone size, visited with i ascending, then j ascending.  The
 * marginals n_i = sum over j and n_j = sum over i, N = sum count, sum i n_i and sum j n_j are exact 64-bit integers; everything after is
 * double, with p = count / N, mu_i = (sum i n_i) / N and mu_j = (sum j n_j) / N:
 *     short_emphasis = (sum n_j / j^2) / N; long_emphasis = (sum n_j j^2) / N; low_grey_emphasis = (sum n_i / i^2) / N;
 *     high_grey_emphasis = (sum n_i i^2) / N; short_low = (sum c / (i^2 j^2)) / N; short_high = (sum c i^2 / j^2) / N;
 *     long_low = (sum c j^2 / i^2) / N; long_high = (sum c i^2 j^2) / N; grey_nonuniformity = (sum n_i^2) / N and _norm = that / N;
 *     size_nonuniformity = (sum n_j^2) / N and _norm = that / N; percentage = N / (voxels * directions), directions = 1 for zones;
 *     grey_variance = sum (i - mu_i)^2 p; size_variance = sum (j - mu_j)^2 p; entropy = - sum p log2 p.
 *   All 16 are NaN when N = 0.  mi_unet_volume_zones_run_features takes one row rlm[r] or rlm_axial[r] and directions 13 or 4;
 *   mi_unet_volume_zones_zone_features takes nz records, uses only those with component == r (the whole list or a slice) and sorts them
 *   by (level, size) itself.
 * MI_UNET_EARG, output untouched: a null c, table, list (with nz > 0) or out; nz < 0; voxels < 1; L or R outside its range; directions
 * not 13 or 4; a zone record of r whose level is outside 0 .. L - 1 or whose size is below 1.
 * There is no group form: mi_unet_group_handle(g, rank) hands out an engine to call this on. */
#define MI_UNET_VZONES_MAX_RUN 8192
#define MI_UNET_VZONES_MAX_CAP 16777216         /* 2^24 */
typedef struct mi_unet_vzones_opts { int mode, levels, lo, width, max_run; } mi_unet_vzones_opts;  /* default { MI_UNET_VTEX_COUNT, 32, 0, 1, 32 } */
typedef struct mi_unet_vzones {        /* 56 bytes, no padding */
    int32_t voxels, imin, imax;        /* voxels with this id; min / max of intensity over them */
    int32_t longest_run;               /* over the 13 offsets, unclamped; 0 without rlm */
    int32_t zones, largest_zone;       /* zones of this component and the voxels of its largest; 0 without zones */
    int64_t runs, runs_axial;          /* sums of rlm[r] and of rlm_axial[r]; 0 for a table that was not asked for */
    int64_t clamped, clamped_axial;    /* runs longer than R in each */
} mi_unet_vzones;
typedef struct mi_unet_vzone { int32_t first, component, level, size; } mi_unet_vzone;     /* 16 bytes */
typedef struct mi_unet_vzone_features {        /* 128 bytes: 16 doubles */
    double short_emphasis, long_emphasis, low_grey_emphasis, high_grey_emphasis, short_low, short_high, long_low, long_high,
           grey_nonuniformity, grey_nonuniformity_norm, size_nonuniformity, size_nonuniformity_norm, percentage, grey_variance,
           size_variance, entropy;
} mi_unet_vzone_features;
int mi_unet_volume_zones(mi_unet_t *h, const int32_t *ids /* [D][H][W] host */, const uint16_t *intensity /* [D][H][W] host */, int D, int H,
                         int W, int m, const mi_unet_vzones_opts *opts, mi_unet_vzones *table /* [m] */,
                         uint32_t *rlm /* [m][L][R] or NULL */, uint32_t *rlm_axial /* [m][L][R] or NULL */,
                         mi_unet_vzone *zones /* [cap] or NULL */, int cap, int *found /* NULL iff zones is NULL */);
int mi_unet_volume_zones_host(const int32_t *ids, const uint16_t *intensity, int D, int H, int W, int m, const mi_unet_vzones_opts *opts,
                              mi_unet_vzones *table, uint32_t *rlm, uint32_t *rlm_axial, mi_unet_vzone *zones, int cap, int *found);
int mi_unet_volume_zones_run_features(const mi_unet_vzones *c, const uint32_t *rlm_row /* [L][R] */, int L, int R, int directions /* 13 or 4 */,
                                      mi_unet_vzone_features *out);
int mi_unet_volume_zones_zone_features(const mi_unet_vzones *c, const mi_unet_vzone *zones, int nz, int r, int L, mi_unet_vzone_features *out);

/* ---- Volume neighbourhoods: per component of a labelled stack its neighbourhood-difference (NGTDM), dependence (NGLDM)
 * and distance-zone (GLDZM) tables
 * A stage of its own, not a setting: nothing else in this header changes behaviour because of it.  Everything up to the feature function
 * is an exact integer count and independent of the order of evaluation.
 * Input is ids, int32 [D][H][W], intensity, uint16 [D][H][W], and the number of components m, as mi_unet_volume_zones takes them; both
 * buffers are required.
 *   COMPONENT  exactly as in mi_unet_volume_texture: component r, 0 <= r < m, is the set of voxels with ids == r + 1.  0, -1 and anything
 *              above m belong to no component.  An id that no voxel carries gives an all-zero entry and all-zero rows.
 *   OPTIONS    opts = { mode, levels L, lo, width, alpha, max_dist Dm }; NULL is { MI_UNET_VTEX_COUNT, 32, 0, 1, 0, 32 }.
 *   LEVEL      mode, L, lo and width mean what they mean in mi_unet_vtexture_opts, and the level of a voxel is mi_unet_volume_texture's
 *              formula: the same stack at the same options has the same levels in all three stages.  A voxel's KEY is
 *              (r + 1) << 8 | level, 0 for a voxel of no component.
 *   NEIGHBOURS N26(p) is the set of voxels among the 26 neighbours of p that lie inside the volume and in p's component; N8(p) is the
 *              same over the 8 neighbours with dz = 0 (what a thick-slice series wants, as glcm_axial and rlm_axial are).  For a voxel
 *              of level l (from 0) with c = |N| and S = the sum of the levels of N:
 *                  ngt_count[r][l][c] += 1                uint32 [m][L][27], c = 0 .. 26
 *                  ngt_diff [r][l][c] += |c l - S|        uint64 [m][L][27]; the column c = 0 stays 0
 *                  dep      [r][l][k] += 1                uint32 [m][L][27], k = the voxels of N whose level differs from l by at most
 *                                                         alpha; the dependence j = k + 1 is column k
 *              and the same over N8 in ngt_count_axial, ngt_diff_axial and dep_axial, [m][L][9].  The tables hold more than the IBSI's
 *              matrices and determine them exactly: n_i = sum over c >= 1 of count, s_i = sum over c >= 1 of diff / c; a voxel with no
 *              neighbour in its component is left out, as the IBSI prescribes; |c l - S| does not depend on whether levels count from 0
 *              or from 1.
 *   DISTANCE   for a voxel p of component r, d(p) = the minimum of |px - qx| + |py - qy| + |pz - qz| over all positions q that are not
 *              in component r, positions outside the volume included: a voxel at the volume's border has d = 1.  This is the IBSI's
 *              6-connected distance.  d_axial(p) is the same inside p's slice: |px - qx| + |py - qy|, q in the slice or outside it in x
 *              or y.
 *   ZONES      a zone is mi_unet_volume_zones': a 26-connected set of voxels with one key that is not 0.  A zone's distance is the
 *              minimum of d over its voxels.  dzm[r][l][min(distance, Dm) - 1] counts zones, uint32 [m][L][Dm]; dzm_axial takes d_axial
 *              over the same 3-D zones.  The last bin collects every distance >= Dm; the entry's `clamped` says how many zones lay
 *              deeper than Dm, so 0 there means the table is the unclamped matrix.
 *   ENTRY      voxels, imin, imax as in mi_unet_vtexture; valid and valid_axial, the voxels with c >= 1 in N26 and in N8 (the sums of
 *              the two count tables without their column 0); zones, the zones of the component; deepest and deepest_axial, the maximum
 *              of d and of d_axial over the component: the radius of its largest inscribed L1 ball; clamped and clamped_axial;
 *              dependence_max, the largest j with a count in dep.
 *   OUTPUT     every table pointer travels in one mi_unet_vnbhood_out; out == NULL is the struct of eight NULLs.  Each pointer may be
 *              NULL: that table is not computed and the entry's fields that belong to it are 0 (valid with ngt_count, valid_axial with
 *              ngt_count_axial, dependence_max with dep, deepest and clamped with dzm, deepest_axial and clamped_axial with dzm_axial,
 *              zones with either).  ngt_count and ngt_diff are both given or both NULL, and so are the axial two.  Without dzm and
 *              dzm_axial the zone half and both distance transforms are skipped.
 * Limits, each with its reason:
 *   D, H, W in 1 .. MI_UNET_SCORE_VOLUME_MAX_SIDE (8192): a distance along a row is below 2^16;
 *   D * H * W <= 2^28: a count cell stays below 2^28 and an index is an int32_t; a diff cell stays below 26 * 63 * 2^28 < 2^40, hence
 *           64 bits;
 *   L in 2 .. MI_UNET_VTEX_MAX_LEVELS (64): the key's 8 level bits, and mi_unet_volume_texture's limit;
 *   alpha in 0 .. L - 1: at L - 1 every neighbour depends; Dm in 1 .. MI_UNET_VNBHOOD_MAX_DIST (4096): no voxel of a volume with sides
 *           of at most 8192 lies deeper;
 *   m in 1 .. MI_UNET_VOLUME_MAX_TABLE and m * L * max(L, 32, Dm) <= MI_UNET_VTEX_MAX_CELLS (2^22): mi_unet_volume_texture's key step
 *           takes m * L * L at once, and no table passes 32 MiB (27 columns of 8 bytes are fewer bytes than 32 of 8);
 *   width in 1 .. 65536 and lo in 0 .. 65535: the range of a uint16_t; a mode that exists.
 * mi_unet_volume_nbhood takes host buffers of any size; its workspace grows on demand, belongs to the handle and is freed by
 * mi_unet_destroy.  It needs the device, not the network: it works before weights are loaded.  It changes no setting and nothing
 * mi_unet_last_regions or mi_unet_last_stage_ms report.  MI_UNET_EARG with a message that begins "mi_unet_volume_nbhood:", nothing queued
 * and no output written: a null ids, intensity or table; one of a count / diff pair without the other; any limit broken.  A workspace
 * that cannot be allocated is MI_UNET_EHIP with a message; the handle stays usable.
 * mi_unet_volume_nbhood_host is the definition as sequential host arithmetic (needs no device), same arguments without the handle, same
 * bytes; its messages begin "mi_unet_volume_nbhood_host:".
 * mi_unet_volume_nbhood_derive is pure host arithmetic in double with a fixed order of summation.  It takes the entry of one component,
 * `rows`: the pointers to that component's rows (ngt_count + r * L * 27 and so on; a NULL row is an absent matrix), L, Dm and `axial`:
 * 0 reads the three N26 rows and dzm, anything else the three N8 rows and dzm_axial (the pointers of the other form are not read).
 * Levels are numbered i = 1 .. L.
 *   NGTDM  with n_i and s_i as above (s_i summed with c ascending), N = sum n_i, p_i = n_i / N and G = the levels with n_i > 0, sums over
 *          i and over (i, j) ascending, pairs only over levels with p_i != 0 and p_j != 0:
 *              coarseness = 1 / sum p_i s_i, 1e6 when that sum is 0 (pyradiomics' convention);
 *              contrast   = (sum_i sum_j p_i p_j (i - j)^2) / (G (G - 1)) * (sum s_i) / N, 0 when G = 1;
 *              busyness   = (sum p_i s_i) / (sum_i sum_j |i p_i - j p_j|), 0 when the denominator is 0;
 *              complexity = (1 / N) sum_i sum_j |i - j| (p_i s_i + p_j s_j) / (p_i + p_j);
 *              strength   = (sum_i sum_j (p_i + p_j) (i - j)^2) / (sum s_i), 0 when sum s_i = 0.
 *          All five are NaN when N = 0 or the pair of rows is absent.
 *   NGLDM and GLDZM  the 16 features of mi_unet_vzone_features by the formulas of the block above, over the non-zero cells (i, j, count)
 *          with i = level + 1 and j = the dependence (column + 1) or the zone distance (bin + 1); percentage = N / voxels.
 *          dependence_energy = sum p^2 over the dependence matrix.  All are NaN for an empty or absent matrix.
 * MI_UNET_EARG, output untouched: a null c, rows or out; voxels < 1; L or Dm outside its range; a count row without its diff row.
 * There is no group form: mi_unet_group_handle(g, rank) hands out an engine to call this on. */
#define MI_UNET_VNBHOOD_MAX_DIST 4096
typedef struct mi_unet_vnbhood_opts { int mode, levels, lo, width, alpha, max_dist; } mi_unet_vnbhood_opts;  /* default { MI_UNET_VTEX_COUNT, 32, 0, 1, 0, 32 } */
typedef struct mi_unet_vnbhood {       /* 44 bytes, no padding */
    int32_t voxels, imin, imax;        /* voxels with this id; min / max of intensity over them */
    int32_t valid, valid_axial;        /* voxels with a neighbour of their component among the 26 / among the 8; 0 without that count table */
    int32_t zones;                     /* zones of this component; 0 without dzm and dzm_axial */
    int32_t deepest, deepest_axial;    /* the maximum of d / of d_axial; 0 without dzm / dzm_axial */
    int32_t clamped, clamped_axial;    /* zones with a distance above Dm in each */
    int32_t dependence_max;            /* the largest dependence j = k + 1 with a count in dep; 0 without dep */
} mi_unet_vnbhood;
typedef struct mi_unet_vnbhood_out {   /* the tables of a call, or the rows of one component; each may be NULL */
    uint32_t *ngt_count;               /* [m][L][27] */
    uint64_t *ngt_diff;                /* [m][L][27]; NULL iff ngt_count is NULL */
    uint32_t *dep;                     /* [m][L][27] */
    uint32_t *ngt_count_axial;         /* [m][L][9] */
    uint64_t *ngt_diff_axial;          /* [m][L][9]; NULL iff ngt_count_axial is NULL */
    uint32_t *dep_axial;               /* [m][L][9] */
    uint32_t *dzm, *dzm_axial;         /* [m][L][Dm] */
} mi_unet_vnbhood_out;
typedef struct mi_unet_vnbhood_features {      /* 304 bytes: 38 doubles */
    double coarseness, contrast, busyness, complexity, strength;
    mi_unet_vzone_features ngldm;
    double dependence_energy;
    mi_unet_vzone_features gldzm;
} mi_unet_vnbhood_features;
int mi_unet_volume_nbhood(mi_unet_t *h, const int32_t *ids /* [D][H][W] host */, const uint16_t *intensity /* [D][H][W] host */, int D, int H,
                          int W, int m, const mi_unet_vnbhood_opts *opts, mi_unet_vnbhood *table /* [m] */, const mi_unet_vnbhood_out *out);
int mi_unet_volume_nbhood_host(const int32_t *ids, const uint16_t *intensity, int D, int H, int W, int m, const mi_unet_vnbhood_opts *opts,
                               mi_unet_vnbhood *table, const mi_unet_vnbhood_out *out);
int mi_unet_volume_nbhood_derive(const mi_unet_vnbhood *c, const mi_unet_vnbhood_out *rows, int L, int Dm, int axial,
                                 mi_unet_vnbhood_features *out);

/* ---- Volume spatial statistics: per component of a labelled stack where its intensity sits: Moran's I, Geary's C, the
 * intensity-weighted centre, the integrated intensity and the local / global intensity peak ---------------------------------------------
 * A stage of its own, not a setting: nothing else in this header changes behaviour because of it.  These are the IBSI morphology and
 * local-intensity features that need the intensity stack.  Everything but four sums of doubles is an exact integer; millimetres enter
 * only in mi_unet_volume_spatial_derive.
 * Input is ids, int32 [D][H][W] (slice z, row y, column x; D, H, W are arguments, not the engine's tile size), intensity, uint16
 * [D][H][W] (required, as in mi_unet_volume_texture), the number of components m, the spacing as three positive integers
 * spacing_units = { ux, uy, uz } in a unit the caller chooses (mi_unet_score_volume_units finds one for a spacing in millimetres) and
 * opts = { max_voxels, peak_r }.
 *   COMPONENT  as in mi_unet_volume_measure: component r, 0 <= r < m, is the set of voxels with ids == r + 1.  Every other value (0, -1,
 *              anything above m) belongs to no component.  A voxel's index is z * H * W + y * W + x.  An id that no voxel carries gives
 *              an all-zero entry.
 *   SUMS       voxels = A; sx, sy, sz over the integer coordinates; si, sii (the sums of v and v * v), imin, imax over the intensity v;
 *              six, siy, siz = sum v x, sum v y, sum v z (below 2^13 * 2^16 * 2^31 = 2^60).
 *   CENTRE     centre = c = floor((2 si + A) / (2 A)), the integer nearest the mean intensity.  With y = v - c, |mean - c| <= 1/2: nothing
 *              that is derived from the pair sums cancels badly.
 *   PEAKS      the sphere of a voxel p is { p + o : o in B(peak_r) } cut to the volume, B(r) the ball of mi_unet_volume_ball in
 *              spacing_units.  Whether a voxel of the sphere belongs to the component is NOT asked (IBSI).  n(p) is the sphere's voxel
 *              count and s(p) the sum of its intensities; mean a > mean b <=> s_a n_b > s_b n_a, in unsigned 64 bits.
 *              Global peak: over all p of the component the largest mean, ties to the smallest index: gp_sum, gp_n, gp_at = s, n, p.
 *              Local peak: the same over the p of the component with v(p) == imax: lp_sum, lp_n, lp_at.
 *              peak_r == 0 makes both the first voxel that carries imax.  Every component gets its peaks: their cost is linear.
 *   PAIRS      for a component with 2 <= A <= max_voxels (and max_voxels > 0), over the unordered pairs i < j of its voxels, with
 *              d2(i, j) = (dx ux)^2 + (dy uy)^2 + (dz uz)^2 between voxel centres (an int32_t, as in mi_unet_volume_measure; its
 *              conversion to double is exact) and w = 1 / sqrt(d2) in double:
 *                s0 = sum w,  s1 = sum w (y_i + y_j),  s2 = sum w y_i y_j,  s3 = sum w (y_i - y_j)^2.
 *              The integer factors are formed exactly and converted once; w is within 4 ulp of the real 1 / sqrt(d2) in either form.
 *              pairs = A (A - 1) / 2 and searched = 1.  A component above the cap, or with A < 2, has searched = 0, pairs = 0 and the
 *              four doubles 0.0; everything else in its entry stays valid.  The cap acts on voxels, a defined quantity, so the two
 *              forms agree on who is skipped.  The four doubles depend on the order of summation: the two forms agree within
 *              2 (P + 8) eps sum |term| for P pairs; the device form gives the same bits from call to call.
 * Limits, each with its reason:
 *   those of mi_unet_volume_measure: D, H, W in 1 .. MI_UNET_SCORE_VOLUME_MAX_SIDE; D * H * W < 2^31; m in 1 .. MI_UNET_VOLUME_MAX_TABLE;
 *           every unit >= 1 and the squared diagonal of the volume in spacing units below 2^31;
 *   max_voxels in 0 .. MI_UNET_VSPATIAL_MAX_VOXELS_LIMIT = 2^20: 2^39 pairs, the most one component may cost;
 *   peak_r in 0 .. MI_UNET_VOLUME_CLEAN_MAX_R = 46340: r * r < 2^31;
 *   B(peak_r) has (2 ey + 1) (2 ez + 1) <= MI_UNET_VSPATIAL_MAX_BALL_ROWS = 4096 rows (ey = peak_r / uy, ez = peak_r / uz) and at most
 *           MI_UNET_VSPATIAL_MAX_BALL_VOXELS = 2^23 voxels: s < 2^23 * 2^16 = 2^39 and s * n < 2^62, inside 64 unsigned bits.
 * opts == NULL is { 131072, 0 }.
 * mi_unet_volume_spatial takes host buffers of any size; its workspace grows on demand, belongs to the handle and is freed by
 * mi_unet_destroy.  It needs the device, not the network: it works before weights are loaded.  It changes no setting and nothing
 * mi_unet_last_regions or mi_unet_last_stage_ms report.  MI_UNET_EARG with a message, nothing queued and no output written: a null ids,
 * intensity, spacing_units or table; a limit above.  A workspace that cannot be allocated is MI_UNET_EHIP with a message; the handle
 * stays usable.
 * mi_unet_volume_spatial_host is the definition as sequential host arithmetic (needs no device), same arguments without the handle: the
 * same bytes in every integer field; the pairs are summed in index order (i ascending, then j).
 * mi_unet_volume_spatial_derive is pure host arithmetic in double.  A voxel is a box of s = spacing_units * unit_mm millimetres per axis
 * and voxel 0 spans 0 .. 1 of the grid.  With A = voxels:
 *   c*_mm = (sum / A + 0.5) * s of the axis, as mi_unet_volume_measure_derive gives it;
 *   ic*_mm = (si* / si + 0.5) * s of the axis, the intensity-weighted centre; NaN when si == 0;
 *   com_shift_mm = the distance of the two; integrated_intensity = si * (the volume of a voxel in mm^3);
 *   local_peak = lp_sum / lp_n and global_peak = gp_sum / gp_n;
 *   with V = (A * sii - si^2) / A from an exact 128-bit numerator and delta = si / A - c:
 *   morans_i = A / (2 s0) * 2 (s2 - delta s1 + delta^2 s0) / V and gearys_c = (A - 1) / (2 * 2 s0) * 2 s3 / V: IBSI's sums over
 *   ordered pairs written over unordered ones.  Both are NaN when searched == 0 or V == 0.
 * MI_UNET_EARG, output untouched: a null pointer, voxels < 1, a unit < 1, or a unit_mm that is not finite and > 0.
 * There is no group form: mi_unet_group_handle(g, rank) hands out an engine to call this on. */
#define MI_UNET_VSPATIAL_MAX_VOXELS_LIMIT 1048576 /* 2^20 */
#define MI_UNET_VSPATIAL_MAX_BALL_ROWS 4096
#define MI_UNET_VSPATIAL_MAX_BALL_VOXELS 8388608  /* 2^23 */
typedef struct mi_unet_vspatial {      /* 168 bytes, no padding */
    int32_t voxels, searched;          /* voxels with this id; 1 when the pair sums were taken */
    int32_t imin, imax;                /* min / max of intensity over the component */
    int32_t centre, reserved;          /* the integer nearest the mean intensity; 0 */
    int32_t gp_at, lp_at;              /* the voxel index of the global and of the local peak */
    int64_t sx, sy, sz;                /* sums of x, y, z over the component */
    int64_t si, sii;                   /* sum v, sum v*v of the intensity */
    int64_t six, siy, siz;             /* sum v x, sum v y, sum v z */
    int64_t gp_sum, gp_n, lp_sum, lp_n; /* the peak spheres: intensity sum and voxel count */
    int64_t pairs;                     /* A (A - 1) / 2 when searched, else 0 */
    double s0, s1, s2, s3;             /* the pair sums */
} mi_unet_vspatial;
typedef struct mi_unet_vspatial_opts { int max_voxels, peak_r; } mi_unet_vspatial_opts;     /* default { 131072, 0 } */
typedef struct mi_unet_vspatial_metrics {
    double cx_mm, cy_mm, cz_mm, icx_mm, icy_mm, icz_mm, com_shift_mm, integrated_intensity, local_peak, global_peak, morans_i, gearys_c;
} mi_unet_vspatial_metrics;
int mi_unet_volume_spatial(mi_unet_t *h, const int32_t *ids /* [D][H][W] host */, const uint16_t *intensity /* [D][H][W] host */, int D, int H,
                           int W, int m, const int spacing_units[3], const mi_unet_vspatial_opts *opts, mi_unet_vspatial *table /* [m] */);
int mi_unet_volume_spatial_host(const int32_t *ids, const uint16_t *intensity, int D, int H, int W, int m, const int spacing_units[3],
                                const mi_unet_vspatial_opts *opts, mi_unet_vspatial *table);
int mi_unet_volume_spatial_derive(const mi_unet_vspatial *c, const int spacing_units[3], double unit_mm, mi_unet_vspatial_metrics *out);

/* ---- Touching objects split: cores regrown by geodesic distance ----------------------------------------------------
 * Two objects joined by a thin bridge are one component for every stage above.  This stage erodes a plane to its cores, labels the
 * cores and grows them back inside the plane, and hands out the pieces in the layout of mi_unet_volume_components, so that every
 * stage that takes a table or an id stack takes the pieces unchanged.  Exact integers; the bytes do not depend on scheduling.
 *
 * masks, values and n are those of mi_unet_volume_components: plane k is S = { masks == values[k] }, planes are independent.
 * spacing_units = { ux, uy, uz } as mi_unet_volume_clean takes them.  opts = { connectivity, neck_r, min_core }, default { 26, 0, 1 }.
 *   CORES   C = the erosion of S by mi_unet_volume_ball(spacing_units, neck_r), with mi_unet_volume_clean's border rule (only voxels
 *           inside the volume constrain an erosion); a neck_r below every unit is the single voxel and C = S.  The cores are the
 *           components of C under `connectivity` (6, 18, 26); one with fewer than min_core voxels is dropped.  The MARKER of a kept
 *           core is its raster-first voxel index z * H * W + y * W + x.
 *   GROWTH  Two voxels of S adjacent under `connectivity` are joined by a step whose cost is the sum of the units of the axes on
 *           which they differ (a face step in x: ux; an edge step in x and z: ux + uz).  The length of a path inside S is the sum
 *           of its steps.  key(v) = the lexicographic minimum of (length, marker) over all kept cores and all paths inside S from a
 *           voxel of that core to v (core voxels: length 0); v belongs to the piece of that marker.  Ties in length go to the
 *           smaller marker, so the rule is total.
 *   REST    The voxels of S that no kept core reaches: their components under `connectivity` are pieces of their own, with no core.
 * The pieces partition S, every piece is connected under `connectivity`, and inside one component of S either every piece has a
 * core or the component is one coreless piece (DESIGN.md 7.21 proves the three).
 *
 * found[k]    the number of pieces of the plane, always exact.
 * table[k]    [n][cap]: the first min(found, cap) pieces in mi_unet_volume_components' ORDER (voxels descending, `first` ascending);
 *             voxels, first, the bounding box and sx, sy, sz are over the piece; kept = 1; value = values[k]; faces_x / _y / _z
 *             count the faces towards a 6-neighbour that is NOT IN THE PIECE (outside S, outside the volume, or in another piece).
 *             Entries behind found are zero.
 * info[k]     [n][cap], may be NULL: mi_unet_vpiece of the same piece: core_first = the marker or -1 for a coreless piece,
 *             core_voxels, reach = the largest length among the piece's keys (0 for a coreless piece), cut_x / _y / _z = those of the
 *             table's faces whose neighbour is in S but in another piece.
 * ids         [n][D][H][W] int32, may be NULL: 1 + the table index, -1 for a piece beyond cap, 0 outside S.
 * stats[k]    may be NULL: value, in_voxels = |S|, core_voxels = |C|, cores, cores_kept, pieces, coreless, max_reach.
 * rounds      int32 [n], may be NULL: how many rounds of the growth ran for the plane (the host form: 0).  Diagnostic; it depends on
 *             scheduling and is no part of the stage's bytes.
 *
 * MI_UNET_EARG, nothing queued and no output touched:
 *   D, H, W >= 1 and n * D * H * W < 2^31     voxel indices, markers and the forest are int32;
 *   values are bytes, 1 .. MI_UNET_VOLUME_MAX_VALUES of them, none twice     a kernel argument holds them;
 *   units and neck_r in 1 / 0 .. MI_UNET_VOLUME_CLEAN_MAX_R     r * r < 2^31, as in mi_unet_volume_clean;
 *   connectivity one of 6, 18, 26; min_core >= 0; cap in 1 .. MI_UNET_VOLUME_MAX_TABLE     the table is sorted in one workgroup's LDS;
 *   D * H * W * (ux + uy + uz) < 2^33     a shortest path visits a voxel at most once and a step costs at most ux + uy + uz, so every
 *           length stays below 2^33 and a key is (length << 31) | marker in one unsigned 64-bit word; all ones = unreached.
 * A workspace that cannot be allocated is MI_UNET_EHIP and the handle stays usable.  Works before weights are loaded, changes no
 * setting, has no group form (mi_unet_group_handle(g, rank) hands out an engine to call it on).  mi_unet_volume_split_host takes the
 * same arguments without the handle, is sequential (erosion from the definition, flood fill, Dijkstra) and gives the same bytes.
 * mi_unet_volume_split_derive: reach_mm = reach * unit_mm, cut_mm2 = cut_x sy sz + cut_y sx sz + cut_z sx sy for a spacing in mm. */
typedef struct mi_unet_vsplit_opts { int connectivity, neck_r, min_core; } mi_unet_vsplit_opts;     /* default { 26, 0, 1 } */
typedef struct mi_unet_vpiece {        /* 40 bytes, no padding */
    int32_t core_first, core_voxels;
    int64_t reach;
    int64_t cut_x, cut_y, cut_z;
} mi_unet_vpiece;
typedef struct mi_unet_vsplit_stat {   /* 64 bytes: 8 int64 */
    int64_t value, in_voxels, core_voxels, cores, cores_kept, pieces, coreless, max_reach;
} mi_unet_vsplit_stat;
typedef struct mi_unet_vpiece_metrics { double reach_mm, cut_mm2; } mi_unet_vpiece_metrics;
int mi_unet_volume_split(mi_unet_t *h, const uint8_t *masks /* [D][H][W] host */, int D, int H, int W, const int *values, int n,
                         const int spacing_units[3], const mi_unet_vsplit_opts *opts, int32_t *ids /* [n][D][H][W] or NULL */,
                         mi_unet_vcomp *table /* [n][cap] */, mi_unet_vpiece *info /* [n][cap] or NULL */, int cap, int32_t *found /* [n] */,
                         mi_unet_vsplit_stat *stats /* [n] or NULL */, int32_t *rounds /* [n] or NULL */);
int mi_unet_volume_split_host(const uint8_t *masks, int D, int H, int W, const int *values, int n, const int spacing_units[3],
                              const mi_unet_vsplit_opts *opts, int32_t *ids, mi_unet_vcomp *table, mi_unet_vpiece *info, int cap,
                              int32_t *found, mi_unet_vsplit_stat *stats, int32_t *rounds);
int mi_unet_volume_split_derive(const mi_unet_vpiece *p, const double spacing_xyz[3], double unit_mm, mi_unet_vpiece_metrics *out);

/* ---- Component skeletons: topology-preserving thinning to a medial line ----------------------------------------------
 * A tubular or branching component (vessel, airway, duct) is described by its medial line: its length, its calibre, its free ends and
 * branch points, whether it closes into a loop.  This stage peels every component of an id stack down to one voxel of thickness without
 * ever changing its topology, and counts the result.  Exact integers; the bytes do not depend on scheduling.
 *
 * INPUT    ids int32 [D][H][W]; component r (0 <= r < m) is { ids == r + 1 }, what mi_unet_volume_components and mi_unet_volume_split
 *          write.  Every other value belongs to nothing, and so does everything outside the volume.  Two voxels are SAME-OBJECT
 *          NEIGHBOURS when they are 26-adjacent and carry the same id in 1 .. m.  Components are thinned independently in one run and
 *          may touch (ids made under connectivity 6, or of two target values).
 * CODE     The neighbourhood of a voxel p as 26 bits: bit i belongs to the i-th offset (dz, dy, dx) of the raster order
 *          (-1,-1,-1), (-1,-1,0), ... (1,1,1) with (0,0,0) left out, and is set when that neighbour is a same-object neighbour of p.
 * SIMPLE   (26-connected object, 6-connected background; Malandain and Bertrand.)  O = the set bits of the code.  B = the 18-neighbours
 *          of p (offsets with |dz| + |dy| + |dx| <= 2) whose bit is clear.  p is simple iff O is not empty and is one 26-connected
 *          component inside the 26 neighbours, and exactly one 6-connected component of B, connectivity taken inside the 18 neighbours,
 *          holds a face neighbour of p.  It depends on the code alone.
 * END      An end point is an object voxel with exactly one same-object neighbour.
 * SCHEDULE A pass first marks the end points of the current state.  Then six phases run in the order z - 1, z + 1, y - 1, y + 1, x - 1,
 *          x + 1.  Phase d first fixes its candidates: the object voxels whose neighbour in direction d is not a same-object neighbour,
 *          in the state at the phase's start.  Then eight sub-steps s = 0 .. 7 follow; the subfield of a voxel is
 *          (x & 1) | (y & 1) << 1 | (z & 1) << 2.  In sub-step s every candidate of subfield s is deleted at once if it was not marked an
 *          end point at the pass's start and is simple in the current state.  Passes repeat until one deletes nothing.  max_passes > 0
 *          stops after that many passes; stable = 1 iff the last pass that ran deleted nothing.
 *          Two voxels of one subfield are never 26-adjacent, so a sub-step's deletions do not see each other: the parallel deletion
 *          equals a sequential one in any order, only simple points go, and components, tunnels and cavities are preserved.
 * RADIUS   r2[p], for a skeleton voxel p, = the minimum of (dx ux)^2 + (dy uy)^2 + (dz uz)^2 over every voxel q with ids[q] != ids[p]
 *          (the ids as given, before the thinning), the volume wrapped in one layer of "nothing" voxels at index -1 and at D / H / W: a
 *          component that touches the border has a finite radius.
 *
 * opts     { max_passes, radius }, default { 0, 1 }.  radius = 0 leaves r2_min / r2_max / r2_sum zero; with radius = 0 and r2 == NULL no
 *          distance is computed.
 * out_ids  [D][H][W] int32, may be NULL: the id on skeleton voxels, 0 elsewhere.
 * r2       [D][H][W] int32, may be NULL: the radius above on skeleton voxels, 0 elsewhere.
 * table    [m] mi_unet_vskel: voxels_in (of the input), voxels (of the skeleton), ends (one same-object skeleton neighbour), isolated
 *          (none), junctions (three or more), links[c] = the unordered 26-adjacent same-object skeleton pairs of class
 *          c = |dx| + 2 |dy| + 4 |dz| - 1, r2_min / r2_max / r2_sum over the skeleton voxels.  An id no voxel carries: all zero.
 * info     may be NULL: passes (the one that deleted nothing included), deleted (voxels over all passes), stable.  `passes` is part of
 *          the definition: the device, the host form and a sequential reading of SCHEDULE report the same number.
 *
 * MI_UNET_EARG with a message that begins with the entry point's name, nothing queued and no output touched:
 *   a null ids, spacing_units or table;
 *   D, H, W in 1 .. MI_UNET_SCORE_VOLUME_MAX_SIDE and D * H * W < 2^31; m in 1 .. MI_UNET_VOLUME_MAX_TABLE; units >= 1;
 *   ((W + 1) ux)^2 + ((H + 1) uy)^2 + ((D + 1) uz)^2 < 2^31     mi_unet_volume_measure's limit on the wrapped volume: every r2 is int32;
 *   max_passes >= 0; radius 0 or 1.
 * A workspace that cannot be allocated is MI_UNET_EHIP and the handle stays usable.  Works before weights are loaded, changes no
 * setting and nothing that mi_unet_last_regions or mi_unet_last_stage_ms report, has no group form.  mi_unet_volume_skeleton_host takes
 * the same arguments without the handle, follows SCHEDULE voxel by voxel and gives the same bytes.
 *
 * mi_unet_volume_skeleton_derive (pure host arithmetic in double; spacing in mm, unit_mm = the length of a spacing unit):
 *   length_mm      sum over c of links[c] * |offset c * spacing|.  A final skeleton holds no deletable voxel, so its curve portions hold no
 *                  adjacency triangles and the sum is the polyline length there; a junction cluster (voxels that are pairwise adjacent)
 *                  counts every pair and OVER-COUNTS.  A surface skeleton (a closed shell) has no length in this sense.
 *   radius_min_mm, radius_max_mm = sqrt(r2_min / r2_max) * unit_mm; radius_rms_mm = sqrt(r2_sum / voxels) * unit_mm; all three 0 for a component
 *                  without skeleton voxels or a call with radius = 0.
 *   loops          links - voxels + 1 for a component with voxels, else 0: the first Betti number ONLY when the skeleton is a curve (a
 *                  connected graph without adjacency triangles); junction clusters and surfaces make it larger.
 *
 * mi_unet_volume_skeleton_simple / _simple_host: SIMPLE for the codes 32 * first_word .. 32 * (first_word + n_words) - 1, as bits
 * (code c is bit c & 31 of bits[(c >> 5) - first_word]), by the kernels' form of the test and by the host form's.  first_word + n_words
 * <= 2^21.  They are how a test compares the two forms on all 2^26 codes. */
typedef struct mi_unet_vskel_opts { int max_passes, radius; } mi_unet_vskel_opts;   /* default { 0, 1 } */
typedef struct mi_unet_vskel {         /* 112 bytes, no padding */
    int64_t voxels_in, voxels, ends, isolated, junctions;
    int64_t links[7];
    int64_t r2_sum;
    int32_t r2_min, r2_max;
} mi_unet_vskel;
typedef struct mi_unet_vskel_info { int64_t deleted; int32_t passes, stable; } mi_unet_vskel_info;     /* 16 bytes */
typedef struct mi_unet_vskel_metrics { double length_mm, radius_min_mm, radius_max_mm, radius_rms_mm; int64_t loops; } mi_unet_vskel_metrics;
int mi_unet_volume_skeleton(mi_unet_t *h, const int32_t *ids /* [D][H][W] host */, int D, int H, int W, int m, const int spacing_units[3],
                            const mi_unet_vskel_opts *opts, int32_t *out_ids /* [D][H][W] or NULL */, int32_t *r2 /* [D][H][W] or NULL */,
                            mi_unet_vskel *table /* [m] */, mi_unet_vskel_info *info /* or NULL */);
int mi_unet_volume_skeleton_host(const int32_t *ids, int D, int H, int W, int m, const int spacing_units[3], const mi_unet_vskel_opts *opts,
                                 int32_t *out_ids, int32_t *r2, mi_unet_vskel *table, mi_unet_vskel_info *info);
int mi_unet_volume_skeleton_derive(const mi_unet_vskel *c, const double spacing_xyz[3], double unit_mm, mi_unet_vskel_metrics *out);
int mi_unet_volume_skeleton_simple(mi_unet_t *h, uint32_t first_word, uint32_t n_words, uint32_t *bits /* [n_words] host */);
int mi_unet_volume_skeleton_simple_host(uint32_t first_word, uint32_t n_words, uint32_t *bits /* [n_words] */);

/* ---- The branch graph of a skeleton: nodes, branches between them, short spurs pruned --------------------------------------
 * mi_unet_volume_skeleton reports a medial line as totals per component.  This stage splits the line into the NODES where it ends or
 * forks and the BRANCHES between them, each branch with its own length, calibre and the nodes it joins, and can prune short spurs.
 * Exact integers and one total rule: the device, the host form and a reading of this text give the same bytes.
 *
 * INPUT    ids int32 [D][H][W] and m as mi_unet_volume_skeleton writes out_ids: component r is { ids == r + 1 }, every other value is
 *          nothing, and so is everything outside the volume.  ANY id stack is legal: nothing below assumes a thin set.  r2 int32
 *          [D][H][W] or NULL: the skeleton stage's radius field, read only at object voxels.  Same-object neighbours are 7.22's: 26-adjacent
 *          voxels that carry the same id in 1 .. m.  The linear index of voxel (z, y, x) is (z H + y) W + x.
 * CLASS    deg(p) = the number of same-object neighbours of p.  deg 0: ISOLATED; 1: END; 2: BRANCH VOXEL; 3 or more: JUNCTION VOXEL.
 * NODES    Every isolated voxel and every end voxel is a node.  Every 26-connected set of junction voxels of one id (a CLUSTER) is one
 *          node.  A node's `first` is the lowest linear index among its voxels; nodes are numbered 0 .. in increasing `first`.
 * BRANCHES (a) Every 26-connected set of branch voxels of one id is a branch.  Each of its voxels has exactly two neighbours, so the set
 *          is a path or a cycle.  An ATTACHMENT is an (ordered) pair (branch voxel, same-object neighbour that is a node voxel); a path
 *          has exactly two, a cycle none: it is CLOSED.  The branch's key is its lowest-index voxel.
 *          (b) Zero-voxel branches: an end voxel whose only neighbour is a junction voxel makes one, keyed by the end voxel; two end voxels
 *          that are each other's only neighbour make one, keyed by the lower index.  Its two node voxels are its two attachments.
 *          Keys are distinct voxels; branches are numbered 0 .. in increasing key.
 *
 * mi_unet_vbranch (88 bytes): first (the key); att_lo / att_hi = the smaller and the larger linear index of the two attached node voxels
 *          (equal when both attachments meet one voxel), -1 / -1 when closed; r2_sum; id; kind 0 = path, 1 = closed, 2 = zero-voxel;
 *          node_a / node_b = the nodes of att_lo / att_hi (-1 / -1 when closed, equal for a loop back into one cluster); voxels = its
 *          branch voxels; links[c] = its adjacent pairs of class c = |dx| + 2 |dy| + 4 |dz| - 1 (7.22's): every pair of two of its voxels
 *          once, every attachment pair, and for a zero-voxel branch the one pair of its two node voxels.  A pair of two voxels of one
 *          node belongs to no branch.  r2_min / r2_max / r2_sum over the branch voxels; all 0 without r2 or with voxels = 0.
 * mi_unet_vnode (56 bytes): first; sz / sy / sx = the coordinate sums of its voxels; id; kind 0 = isolated, 1 = end, 2 = junction; voxels;
 *          degree = the attachments of all branches at its voxels (a loop counts two); r2_min / r2_max over its voxels (0 without r2).
 * mi_unet_vgraph [m] (128 bytes, per id): nodes, ends, junction_nodes, isolated (nodes by kind), junction_voxels, branches, closed,
 *          links[7] summed over the id's branches, pruned_spurs, pruned_voxels.  Always complete; an id no voxel carries: all zero.
 *          Over every id: the sum of degree = 2 (branches - closed), and branch voxels + node voxels = object voxels.
 * TABLES   The caller gives cap_nodes and cap_branches, each 0 .. MI_UNET_VBRANCH_MAX_ROWS; a cap of 0 with a NULL table is legal.  Rows
 *          0 .. min(found, cap) - 1 are written, no other; info reports found_nodes and found_branches.  node_a / node_b and the values of
 *          `map` are ranks in the full numbering, whatever the caps.
 * map      int32 [D][H][W] or NULL: branch index + 1 on branch voxels, -(node index + 1) on node voxels, 0 elsewhere.
 * out_ids  int32 [D][H][W] or NULL: the ids (outside 1 .. m: 0) after pruning.
 * PRUNING  opts { prune_voxels, prune_rounds }, default { 0, 0 }.  A SPUR is a branch that is not closed, has one node of kind end and the
 *          other of kind junction, and voxels + 1 <= prune_voxels (with prune_voxels = 0 nothing is a spur).  A round builds the graph of
 *          the current state; if it has a spur, the round deletes the branch voxels and the end voxel of EVERY spur of that graph at once;
 *          junction voxels stay.  Rounds repeat until a state has no spur, or until prune_rounds > 0 rounds have deleted.  info.rounds =
 *          the rounds that deleted something; info.stable = 1 iff the final state has no spur.  The reported graph, map and out_ids are
 *          those of the final state: a junction voxel left with two neighbours is then a branch voxel, and the two branches it joined
 *          are one.  A star whose arms are all spurs COLLAPSES to its junction: all its arms go in one round and the junction is left
 *          an isolated node; prune with a smaller prune_voxels, or not at all, where that is not wanted.  pruned_spurs / pruned_voxels
 *          count, per id and over all rounds, the spurs and the voxels deleted (end voxels included).  The result is a set function of
 *          the input: nothing depends on scheduling.  The thinned set is not re-thinned; mi_unet_volume_skeleton on out_ids does that.
 *
 * MI_UNET_EARG with a message that begins with the entry point's name, nothing queued and no output touched:
 *   a null ids, spacing_units or graph; nodes NULL with cap_nodes > 0, branches NULL with cap_branches > 0;
 *   cap_nodes, cap_branches in 0 .. MI_UNET_VBRANCH_MAX_ROWS; prune_voxels, prune_rounds in 0 .. MI_UNET_VBRANCH_MAX_PRUNE;
 *   mi_unet_volume_skeleton's limits on D, H, W, m and spacing_units (which only the derived metrics use).
 * A workspace that cannot be allocated is MI_UNET_EHIP and the handle stays usable.  Works before weights are loaded, changes no
 * setting, has no group form.  mi_unet_volume_branches_host takes the same arguments without the handle, follows the text above voxel
 * by voxel and gives the same bytes.
 *
 * mi_unet_volume_branches_derive_branch (host arithmetic in double; H, W of the volume, spacing in mm, unit_mm as in 7.22):
 *   length_mm = sum over c of links[c] * |offset c * spacing|; chord_mm = the distance from att_lo to att_hi (0 when closed);
 *   tortuosity = length_mm / chord_mm, 0 when closed or when the chord is 0; radius_min_mm / radius_max_mm / radius_rms_mm as 7.22's.
 * mi_unet_volume_branches_derive (g = the row of `id` in the per-id table; branches = the table of the call, n_branches = the rows it
 *   holds, found_nodes = info's): length_mm from g->links, which has no over-count inside clusters; parts = the connected components of
 *   the id's graph, by a union-find over node_a / node_b in which every closed branch and every isolated node is a part of its own;
 *   loops = branches - nodes - closed + parts, the cycle rank.  MI_UNET_EARG when the table holds fewer than g->branches rows of the id:
 *   it was truncated. */
#define MI_UNET_VBRANCH_MAX_ROWS (1 << 20)
#define MI_UNET_VBRANCH_MAX_PRUNE (1 << 20)
typedef struct mi_unet_vbranch_opts { int prune_voxels, prune_rounds; } mi_unet_vbranch_opts;   /* default { 0, 0 } */
typedef struct mi_unet_vbranch {       /* 88 bytes, no padding */
    int64_t first, att_lo, att_hi, r2_sum;
    int32_t id, kind, node_a, node_b, voxels;
    int32_t links[7];
    int32_t r2_min, r2_max;
} mi_unet_vbranch;
typedef struct mi_unet_vnode {         /* 56 bytes, no padding */
    int64_t first, sz, sy, sx;
    int32_t id, kind, voxels, degree, r2_min, r2_max;
} mi_unet_vnode;
typedef struct mi_unet_vgraph {        /* 128 bytes, no padding */
    int64_t nodes, ends, junction_nodes, isolated, junction_voxels, branches, closed;
    int64_t links[7];
    int64_t pruned_spurs, pruned_voxels;
} mi_unet_vgraph;
typedef struct mi_unet_vbranch_info { int64_t found_nodes, found_branches; int32_t rounds, stable; } mi_unet_vbranch_info;    /* 24 bytes */
typedef struct mi_unet_vbranch_metrics { double length_mm, chord_mm, tortuosity, radius_min_mm, radius_max_mm, radius_rms_mm; } mi_unet_vbranch_metrics;
typedef struct mi_unet_vgraph_metrics { double length_mm; int64_t parts, loops; } mi_unet_vgraph_metrics;
int mi_unet_volume_branches(mi_unet_t *h, const int32_t *ids /* [D][H][W] host */, const int32_t *r2 /* [D][H][W] or NULL */, int D, int H, int W,
                            int m, const int spacing_units[3], const mi_unet_vbranch_opts *opts, mi_unet_vnode *nodes /* [cap_nodes] or NULL */,
                            int cap_nodes, mi_unet_vbranch *branches /* [cap_branches] or NULL */, int cap_branches, mi_unet_vgraph *graph /* [m] */,
                            int32_t *map /* [D][H][W] or NULL */, int32_t *out_ids /* [D][H][W] or NULL */, mi_unet_vbranch_info *info /* or NULL */);
int mi_unet_volume_branches_host(const int32_t *ids, const int32_t *r2, int D, int H, int W, int m, const int spacing_units[3],
                                 const mi_unet_vbranch_opts *opts, mi_unet_vnode *nodes, int cap_nodes, mi_unet_vbranch *branches, int cap_branches,
                                 mi_unet_vgraph *graph, int32_t *map, int32_t *out_ids, mi_unet_vbranch_info *info);
int mi_unet_volume_branches_derive_branch(const mi_unet_vbranch *row, int H, int W, const double spacing_xyz[3], double unit_mm,
                                          mi_unet_vbranch_metrics *out);
int mi_unet_volume_branches_derive(const mi_unet_vgraph *g, const mi_unet_vbranch *branches, int64_t n_branches, int64_t found_nodes, int id,
                                   const double spacing_xyz[3], double unit_mm, mi_unet_vgraph_metrics *out);

/* Page-locked host memory.  RAW images handed to mi_unet_infer_raw16 / mi_unet_segment_raw16 (and their group forms) from such
 * a buffer are read by the DMA engine directly -- no staging copy on the calling thread (100 MB for sixteen 2048 x 1536 images:
 * 3 - 5 ms of memcpy that the pageable route pays).  Any hipHostMalloc'd / hipHostRegister'ed pointer is recognised, not only
 * these; ordinary pointers keep working through the engine's own pinned ring. */
int mi_unet_host_alloc(size_t bytes, void **p);
void mi_unet_host_free(void *p);

/* Device time of the stages of the LAST mi_unet_infer_raw16 / mi_unet_segment_raw16 (or tiled) call on this handle, in milliseconds, summed
 * over its micro-batches (hipEvent pairs on the streams the stages run on; the upload / preprocess stage of micro-batch k + 1
 * runs on a second stream under the network of micro-batch k, so the stages may add up to more than the call took).  The
 * reference logs two durations per image (src/process.cpp:223-228, :245-253); these are the terms of its "Inference time". */
#define MI_UNET_STAGE_UPLOAD_PRE 0   /* host staging copy + H2D + min/max + bilinear resample (f1) */
#define MI_UNET_STAGE_NETWORK 1      /* UNet + argmax (graph replay) */
#define MI_UNET_STAGE_POSTPROCESS 2  /* postprocess_mask (f2) */
#define MI_UNET_STAGE_CONTOURS 3     /* mask_to_image + extract_contours (f3) */
#define MI_UNET_STAGE_DOWNLOAD 4     /* D2H of tiles, masks / label maps, contours, logits */
#define MI_UNET_N_STAGES 5
int mi_unet_last_stage_ms(const mi_unet_t *h, float *ms /* [MI_UNET_N_STAGES] */);

/* Use an external hipStream_t (e.g. the caller framework's current stream) instead of the engine's own; NULL restores the engine's
 * own, a non-blocking stream that is NOT ordered against the legacy default stream.  From the next call on, every entry point of
 * the handle enqueues on that stream.
 *  - The switch waits for nothing.  Work the handle enqueued on the stream it leaves keeps running there, and it uses the handle's
 *    activation buffers: before the first call on the new stream the CALLER orders the two -- synchronise the stream being left, or
 *    make the new stream wait on an event recorded on it.  Calls on two streams that are not ordered race on those buffers.
 *  - The stream being left must still exist when mi_unet_set_stream is called (the handle may record an event on it); the caller may
 *    destroy it afterwards, once its work has completed.  The stream that is current when the handle is destroyed, or weights are
 *    loaded, must exist then.
 *  - Graphs are cached per stream (mi_unet_infer_u8_device): coming back to a stream replays what was captured on it.
 * mi_unet_sync waits for the CURRENT stream only, i.e. for the calls made since the last switch, not for a stream left earlier. */
int mi_unet_set_stream(mi_unet_t *h, void *hip_stream);
int mi_unet_sync(mi_unet_t *h);

/* Time the last `mi_unet_infer_u8_device` calls: brackets with hipEvents on the handle's current stream (both on the same one).
 * mi_unet_timer_begin/end return elapsed milliseconds through *ms at end (end synchronises the stop event). */
int mi_unet_timer_begin(mi_unet_t *h);
int mi_unet_timer_end(mi_unet_t *h, float *ms);

/* Per-launch accounting since profiling was last switched on: mi_unet_set_profiling(h,1) clears the log and from then on
 * brackets every kernel launch with a hipEvent pair recorded on the launch stream (no host wait at launch time).
 * mi_unet_get_kernel_stats synchronises the last event, fills up to `cap` entries (launch order) and returns the number
 * of launches logged in *n. */
typedef struct mi_unet_kernel_stat {
    char name[48];        /* layer name, e.g. "up4.c1" */
    char kernel[32];      /* kernel family: conv3x3_mfma, convT2x2_mfma, conv3x3_c1, maxpool2x2, head_argmax */
    double flops;         /* algorithmic FLOPs of this launch (2*MAC) */
    double bytes;         /* algorithmic HBM bytes of this launch (inputs + weights + outputs, each once) */
    float ms;             /* measured duration */
} mi_unet_kernel_stat;
int mi_unet_set_profiling(mi_unet_t *h, int on);
int mi_unet_get_kernel_stats(mi_unet_t *h, mi_unet_kernel_stat *stats, int cap, int *n);

/* Parity hook: run ONE layer kernel on host NHWC fp32 buffers (uploaded, run, downloaded).
 *   op = "conv3x3"  : in [B][H][W][Cin], w [Cout][Cin][3][3], scale/shift [Cout] (folded BN; NULL = 1/0), relu flag
 *   op = "conv3x3_wino" / "conv3x3_wino16" : the same layer through the Winograd F(2x2,3x3) kernels
 *   op = "conv3x3_bf16" / "convT2x2_bf16" / "conv3x3_fp16" / "convT2x2_fp16" : the 16-bit-operand kernels
 *   op = "convT2x2" : in [B][H][W][Cin], w [Cin][Cout][2][2], shift = bias [Cout]  -> out [B][2H][2W][Cout]
 *   op = "maxpool"  : in [B][H][W][Cin]                                          -> out [B][H/2][W/2][Cin]
 *   op = "upsample2x" / "upsample2x_bf16" / "upsample2x_fp16" : in [B][H][W][Cin] -> out [B][2H][2W][Cin], bilinear with
 *                     align_corners=True, Cin % 16 == 0, no weights (the 16-bit ops round the input to 16 bits first)
 *   op = "maxpool_bf16" / "maxpool_fp16" : the 16-bit stand-alone pooling (non-negative values: it orders bit patterns), C % 8 == 0
 *   op = "conv3x3_wino_splitk" / "conv3x3_wino4_splitk" (the suffix stands in front of _pool: "conv3x3_wino4_splitk_pool"; these
 *                     two ops only): the launch gets a split-K workspace, as the engine's plan gives every 3x3 layer -- 8 slabs
 *                     [B][H][W][Cout] of floats, at most 64 MiB, filled with 0xFF bytes, between the call's guards -- and the launcher
 *                     decides as in the plan whether and how often it cuts K.  "_splitk<N>", N = 2 .. 8: a workspace of exactly N
 *                     slabs, which the launcher's split has to shrink to.  The strided entry point reports the route name +
 *                     "+splitk<slices>" when K was split ("conv3x3_wino4+splitk3"), the bare route name when the shape admits no
 *                     split.  A touched workspace guard fails the call.
 * Weights are given in PyTorch layout exactly as in the weight file. */
int mi_unet_layer_debug(int device, const char *op, const float *in, int B, int H, int W, int Cin, const float *w,
                        const float *scale, const float *shift, int Cout, int relu, float *out);

/* The same launch in a strided layout, to see every byte the kernel was NOT supposed to touch: the engine's tensors are halves of
 * concat buffers (pixel stride 2 * Cout, first output channel 0 or Cout).  Strides in elements, 0 = the dense default:
 *   ldc     pixel stride of the input           (>= Cin;  the first layer reads the u8 image and has none)
 *   ldo     pixel stride of the output          (>= co_off + Cout; maxpool writes dense and has none)
 *   co_off  first output channel written        (>= 0;    conv, transposed conv and upsample only)
 *   pool_ld pixel stride of the pooled output   (>= Cout; the _pool forms only)
 *   guard_bytes  a guard of that size in front of and behind every device tensor of the call (input, output, pooled output); a
 *           multiple of 256.
 * The whole output and pooled allocations are filled with 0xFF bytes (a NaN in fp32, bf16 and fp16) before the launch, and so are
 * the input's guards and its gap channels [Cin, ldc).  A layout outside these bounds, or one the route's own launcher refuses, is an
 * error and nothing is launched.  out_raw receives the complete output allocation -- guard, [npix][ldo] elements, guard -- as raw
 * bytes, nothing converted; pool_raw the pooled one for the _pool forms (NULL otherwise).  info: the element size, the two
 * allocation sizes and the name of the route that ran (as mi_unet_layer_info::kernel).  A capacity that is too small is an error
 * with info filled in. */
typedef struct mi_unet_debug_layout {
    int ldc, ldo, co_off, pool_ld;
    long long guard_bytes;
} mi_unet_debug_layout;
typedef struct mi_unet_debug_strided_info {
    int elem_bytes;           /* bytes per output element: 4, or 2 for the 16-bit outputs */
    unsigned long long out_bytes, pool_bytes;   /* the whole allocations, guards included (pool_bytes 0 without _pool) */
    char kernel[32];
} mi_unet_debug_strided_info;
int mi_unet_layer_debug_strided(int device, const char *op, const float *in, int B, int H, int W, int Cin, const float *w,
                                const float *scale, const float *shift, int Cout, int relu, const mi_unet_debug_layout *layout,
                                void *out_raw, size_t out_cap, void *pool_raw, size_t pool_cap, mi_unet_debug_strided_info *info);

/* Numeric guard of the default fp32 plan (conv_algo auto / winograd).  Winograd F(4x4,3x3) is exact arithmetic re-associated:
 * its rounding error relative to a layer's operand range is about five times that of F(2x2,3x3) (2e-5 against 4e-6 on logits
 * of magnitude 4), and the path's bar is absolute (logits within 1e-3 of the fp32 reference, BASELINE north_star).  Whether
 * F(4x4) holds that bar therefore depends on the dynamic range of the loaded weights.  Guarantee: when weights are loaded, one
 * probe tile runs through the plan with every 3x3 layer on F(4x4) and again with every 3x3 layer on F(2x2); if the logits differ
 * by more than 5e-4 (half the bar; the difference of the two plans overstates either one's own error), this handle -- and its clones -- runs F(2x2,3x3) on every layer.  The returned
 * text says which (the facade logs it); *tripped / *diff (may be NULL) receive the decision and the measured difference.
 * The same text reports the one other thing that can change a handle's kernels behind the caller's back: when the code objects of
 * the two assembly kernels (conv3x3_wino4a, conv3x3_wino4b) were wanted and could not be loaded at mi_unet_create -- a failed
 * load or symbol look-up, a device that is not gfx950 -- it ends with "; assembly kernels not available (<reason>): ..." and the
 * handle and its clones run those layers on the hipcc F(4x4,3x3) kernels, as under MIUNET_WINO4_ASM=0.
 * Beyond logits of magnitude ~1e2 no fp32 algorithm holds an ABSOLUTE 1e-3 (fp32 itself resolves 6e-8 of the range per
 * operation); there the guard still picks the tighter algorithm and the meaningful bound is relative (~1e-6 of the range). */
const char *mi_unet_numeric_guard(const mi_unet_t *h, int *tripped, float *diff);

/* In-situ parity hook (tests): what the engine's OWN launch plan does to its OWN activations, layer by layer, at any size.
 * The opaque seam this opens is the reference's graph replay (src/process.cpp:143-155), whose intermediate tensors nobody
 * can see.  A "layer" is one step of the plan in launch order (inc.c1, inc.c2, down1.pool, down1.c1, ... outc+argmax);
 * steps whose work is fused into their producer (pooling, the head) are listed and flagged `skipped`.
 *   mi_unet_debug_layer_count : number of steps
 *   mi_unet_debug_layer_info  : static description of step `layer` (shapes are per image)
 *   mi_unet_debug_capture     : uploads B <= max_batch images, runs the plan EAGERLY with exactly the kernels a batch of B
 *       takes, stops after step `layer`, and returns for image `img` of the batch, converted to float, dense NHWC:
 *         in     [in_h][in_w][in_c]      the tensor the step's kernel read (u8 image values 0..255 for the first layer)
 *         out    [out_h][out_w][out_c]   what it stored; when the step ran the fused 1x1 head instead (info->fused_head),
 *                                        the planar logits [classes][out_h][out_w]
 *         pooled [out_h/2][out_w/2][out_c] the fused 2x2 max-pooled tensor (only when info->pooled; may be NULL)
 *         labels [out_h][out_w]          argmax labels (only for head / fused-head steps; may be NULL)
 *       and in *info the dynamic facts: kernel family launched, storage width of the tensors in HBM, flags. */
typedef struct mi_unet_layer_info {
    char name[48];
    char kernel[32];       /* kernel family launched (capture only) */
    int kind;              /* 0 first conv, 1 conv3x3, 2 convT2x2, 3 maxpool2x2, 4 head+argmax, 5 bilinear x2 upsample
                              (bilinear decoder: in = the low-resolution tensor, out = the concat slice it wrote) */
    int in_h, in_w, in_c;
    int out_h, out_w, out_c;
    int in_bits, out_bits; /* 8 = u8 image, 16 = bf16 / fp16 (per conv_algo), 32 = fp32: storage type in HBM (capture only) */
    int pooled;            /* the step also stored the 2x2 max-pooled tensor */
    int fused_head;        /* the step ran the 1x1 head + argmax in its epilogue; its own activations never reached HBM */
    int skipped;           /* not launched at this batch size: fused into its producer (pooling, head) or its consumer (first layer) */
    int fused_first;       /* the step computed the network's first layer in its loader: `in` of the capture is the u8 image */
} mi_unet_layer_info;
int mi_unet_debug_layer_count(const mi_unet_t *h);
int mi_unet_debug_layer_info(const mi_unet_t *h, int layer, mi_unet_layer_info *info);
int mi_unet_debug_capture(mi_unet_t *h, const uint8_t *imgs, int B, int layer, int img, float *in, float *out, float *pooled,
                          uint8_t *labels, mi_unet_layer_info *info);

/* A second context on the SAME device that shares the source engine's weight blob (no second copy, no re-packing) but
 * owns its activation buffers, stream and graphs -- the counterpart of the reference's per-thread TensorRTContext over one
 * shared ICudaEngine (include/process.h:13-26, src/process.cpp:15, :69).  max_batch <= 0 keeps the source's.  The weights
 * stay alive until the last handle that shares them is destroyed, in any order; so do the assembly kernels' code objects, which
 * mi_unet_create loaded for the device.  A clone also keeps the source's MIUNET_* switches as the source parsed them at create. */
int mi_unet_clone(const mi_unet_t *src, int max_batch, mi_unet_t **out);

/* Waits for every stream the handle launched on (a stream given to mi_unet_set_stream included: it must still exist), then frees
 * what the handle owns and drops its share of the weights and code objects.  The library keeps nothing per process. */
void mi_unet_destroy(mi_unet_t *h);

/* ---- Multi-device group (the slot is the reference's sequential file loop, src/main.cpp:148-164) -------------
 * One engine handle + one host worker thread per device inside ONE process.  The path shards by image: a batch of B
 * images is cut into contiguous ranges (rank r of R owns [r*q + min(r, B%R), ...), the first B%R ranks one image more) and
 * every rank runs its range independently -- no collective inside the forward pass.  Two exchange steps exist:
 *   weights : parsed, BN-folded and packed ONCE on the host, uploaded to the first device, then sent to the other devices
 *             device-to-device: ncclBroadcast over xGMI (RCCL, loaded with dlopen when the group spans > 1 distinct device)
 *             or a peer copy when RCCL is unavailable / two ranks share a device;
 *   labels  : MI_UNET_GATHER_HOST (default): every rank copies its own range straight into the caller's host buffer (its own
 *             PCIe link, no collective);  MI_UNET_GATHER_XGMI: grouped ncclSend / ncclRecv of the u8 label maps into the
 *             first device (7 concurrent point-to-point transfers on an 8-GPU node), then one D2H.
 * `devices` lists HIP ordinals, one rank each (a repeated ordinal puts two ranks on one GPU: a test configuration, peer-copy
 * weights, HOST gather only); devices == NULL means ordinals cfg->device .. cfg->device + n_devices - 1, and n_devices <= 0
 * means every visible device.  cfg->max_batch is per rank.  N > 1 distinct devices has never run on hardware here; the RCCL code path
 * itself (communicators, broadcast, send / recv gather) runs in the tests on one card against a stand-in library (MIUNET_RCCL_LIB,
 * MIUNET_GROUP_RCCL=2: tests/cpu/fake_rccl.cpp). */
typedef struct mi_unet_group mi_unet_group_t;
#define MI_UNET_GATHER_HOST 0
#define MI_UNET_GATHER_XGMI 1
int mi_unet_group_create(const mi_unet_config *cfg, const int *devices, int n_devices, mi_unet_group_t **out);
/* A second set of contexts over the same devices that shares every rank's weight blob (mi_unet_clone per rank) and owns its
 * buffers, streams and worker threads: two groups can have two batches in flight at once -- the small serial stages of one
 * (RAW upload, preprocessing, labelling, the contour walk) overlap the network of the other.  The clone has no RCCL
 * communicator (host gather only). */
int mi_unet_group_clone(mi_unet_group_t *src, mi_unet_group_t **out);
int mi_unet_group_size(const mi_unet_group_t *g);
mi_unet_t *mi_unet_group_handle(mi_unet_group_t *g, int rank);            /* rank's engine (owned by the group) */
int mi_unet_group_load_weights(mi_unet_group_t *g, const char *path);
int mi_unet_group_load_weights_from_memory(mi_unet_group_t *g, const void *blob, size_t len);
int mi_unet_group_set_gather(mi_unet_group_t *g, int mode);               /* EARG when XGMI is asked for without RCCL */
int mi_unet_group_set_postprocess(mi_unet_group_t *g, int on);
/* how the weights reached ranks > 0 -- "rccl", "peer-copy" or "host-upload", with the reason when a faster transport failed
 * and the next one was taken -- and the gather mode in force */
const char *mi_unet_group_weight_transport(const mi_unet_group_t *g);
int mi_unet_group_gather(const mi_unet_group_t *g);
/* Sharded forms of mi_unet_infer_u8 / mi_unet_infer_raw16 / mi_unet_segment_raw16: same arguments, same results, the batch
 * split across the group's ranks. */
int mi_unet_group_infer_u8(mi_unet_group_t *g, const uint8_t *imgs, int B, uint8_t *labels, float *logits);
int mi_unet_group_infer_raw16(mi_unet_group_t *g, const uint16_t *const *raws, const int *widths, const int *heights, int B,
                              uint8_t *tiles, uint8_t *labels, float *logits);
int mi_unet_group_segment_raw16(mi_unet_group_t *g, const uint16_t *const *raws, const int *widths, const int *heights, int B,
                                uint8_t *tiles, uint8_t *masks, int32_t *xy, int cap_points, int32_t *start, int cap_contours,
                                int32_t *counts);
/* mi_unet_set_targets on every rank (all or none), and the sharded form of mi_unet_segment_raw16_multi: same arguments, same results */
int mi_unet_group_set_targets(mi_unet_group_t *g, const mi_unet_target *t, int n);
int mi_unet_group_segment_raw16_multi(mi_unet_group_t *g, const uint16_t *const *raws, const int *widths, const int *heights, int B,
                                      uint8_t *tiles, uint8_t *masks, int32_t *xy, int cap_points, int32_t *start, int cap_contours,
                                      int32_t *counts);
/* mi_unet_set_morph on every rank (all or none); mi_unet_group_segment_raw16_multi then applies it */
int mi_unet_group_set_morph(mi_unet_group_t *g, const mi_unet_morph *m, int n);
/* mi_unet_set_window on every rank (all or none); the sharded RAW-in calls above then apply it */
int mi_unet_group_set_window(mi_unet_group_t *g, const mi_unet_window *w);
/* mi_unet_set_measure on every rank (all or none); mi_unet_last_regions of the last sharded segment call: same arguments, the planes in
 * image order, assembled from the ranks' shard ranges */
int mi_unet_group_set_measure(mi_unet_group_t *g, const mi_unet_measure *m);
int mi_unet_group_last_regions(const mi_unet_group_t *g, mi_unet_region *regions, int32_t *counts, int cap_planes, int *planes,
                               int *cap_contours);
void mi_unet_group_destroy(mi_unet_group_t *g);
/* The split itself (pure host arithmetic, needs no device): rank's range [*lo, *hi) of n_items over `world` ranks. */
int mi_unet_shard_range(int n_items, int rank, int world, int *lo, int *hi);

/* Message of the last failing call on this thread ("" if none). */
const char *mi_unet_last_error(void);

/* Number of visible HIP devices (0 when there is no driver); never fails. */
int mi_unet_device_count(void);

#ifdef __cplusplus
}
#endif
#endif /* MI_UNET_H */
