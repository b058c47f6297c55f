// engine_internal.h -- the weight containers and packing functions of weights.cpp, and what group.cpp (the multi-device group of
// include/mi_unet.h) needs from engine.cpp.  Internal to libmiunet.so.
#pragma once
#include <hip/hip_runtime.h>

#include <memory>
#include <string>
#include <vector>

#include "../../include/mi_unet.h"

namespace miunet {

// The decoder's upsampling (weight-file version 2, miunet/spec.py): 2x2 transposed conv (version 1 files) or parameter-free
// bilinear x2 with align_corners=True followed by narrower convolutions (Pytorch-UNet's bilinear=True)
enum : int { UP_TRANSPOSE = 0, UP_BILINEAR = 1 };

// Weights after BN folding and repacking, in device layout, still on the host: one contiguous blob (one upload or one
// broadcast) plus the offsets the launch plan points at.
struct HostWeights {
    std::vector<float> blob;
    struct Off { size_t w, shift, w4; };        // w4: second packing of the same layer (F(4x4) / per-tap kernels), 0 = none
    std::vector<Off> conv;                      // per 3x3 conv in file order (first one = first-layer layout)
    std::vector<Off> convT;                     // empty for the bilinear decoder
    Off head{};
    int up_mode = UP_TRANSPOSE;                 // the decoder the file describes (weight-file version 2's up_mode)
};

// The device copy of that blob.  Shared (std::shared_ptr) by a handle and its clones; freed with the last of them.
struct DeviceWeights {
    int device = 0;
    float *d = nullptr;
    size_t floats = 0;
    HostWeights layout;                         // offsets only (blob left empty)
    ~DeviceWeights();
};

int engine_fail(int code, const std::string &msg);                 // sets this thread's mi_unet_last_error() (weights.cpp)
const std::string &engine_last_error();                            // ... and reads it back

// ---- weights.cpp: host-only, no HIP call
size_t round_up(size_t v, size_t g);
uint16_t bf16_bits(float x);                                       // round-to-nearest-even, as the device converts activations
uint16_t fp16_bits(float x);
float bf16_to_float(uint16_t b);
float fp16_to_float(uint16_t h);
void first_layer_lut(float lut[256]);                              // i / 255.0f
// The packed layouts the kernels read.  FIRST [tap][ci][co]; MFMA / MFMA_T fp32 conv3x3 / convT2x2; TAPS per-tap convT; WINO,
// WINO16 F(2x2,3x3); WINO4 F(4x4,3x3); LP / LP_T the 16-bit conv3x3 / convT2x2.  NONE and UP (pooling, upsampling) have no weights.
enum class Pack { NONE, FIRST, MFMA, MFMA_T, TAPS, WINO, WINO16, WINO4, LP, LP_T, UP };
size_t packed_npad(Pack p, int cout);                              // the padded N a launch passes as ConvArgs::CoutPad
size_t packed_floats(Pack p, int cin, int cout);                   // size of the packed tensor, in floats
// w: PyTorch [Cout][Cin][3][3] (conv) or [Cin][Cout][2][2] (convT); scale: per-channel BN scale folded in double before any
// rounding (null = 1; the transposed layouts take none); fp16: LP / LP_T round to binary16 instead of bfloat16; dst: zero-filled
void pack_weights(Pack p, bool fp16, const float *w, const double *scale, int cin, int cout, float *dst);
// parse "MIUNETW1" (version 1, or 2 with its up_mode), fold BN, repack for `algo` (a resolved MI_UNET_CONV_* value, see engine_algo)
// (weights.cpp)
int engine_pack_weights(const mi_unet_config &cfg, int algo, const void *blob, size_t len, HostWeights &hw);
// allocate the device blob of `h` for `hw` (uploading hw.blob when `upload`, else leaving the bytes to the caller: a
// broadcast or a peer copy fills engine_weight_ptr()), then build the launch plan
int engine_adopt_weights(mi_unet_t *h, const HostWeights &hw, bool upload);
// the numeric guard of the default fp32 plan, run once the weight bytes are on the device (engine.cpp)
int engine_calibrate(mi_unet_t *h);
float *engine_weight_ptr(mi_unet_t *h);
size_t engine_weight_floats(const mi_unet_t *h);
int engine_algo(const mi_unet_t *h);
const mi_unet_config &engine_config(const mi_unet_t *h);
hipStream_t engine_stream(const mi_unet_t *h);

}  // namespace miunet
