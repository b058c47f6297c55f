// plan.h -- the forward pass as a list of steps (build_plan, once per weight set) and each step's launch for one micro-batch
// (route_plan: routing.cpp decides the kernel, the plan fills in the arguments and the fusions it asks for).  Host code only
// (plan.cpp): the buffer addresses are carried, never dereferenced, so the CPU tests build the real plan with made-up ones.
// Internal to libmiunet.so.
#pragma once
#include <string>
#include <vector>

#include "engine_internal.h"
#include "routing.h"

namespace miunet {

struct Step {
    enum Kind { FIRST, CONV, CONVT, POOL, HEAD, UPSAMPLE } kind;
    std::string name;
    ConvArgs a{};                 // CONV / CONVT
    // FIRST / POOL / HEAD / UPSAMPLE operands (UPSAMPLE: src [H][W][C] -> channels [co_off, co_off + C) of dst [2H][2W][ld])
    const float *src = nullptr;
    float *dst = nullptr;
    const float *w = nullptr, *shift = nullptr;
    int H = 0, W = 0, C = 0, Cout = 0, ld = 0, co_off = 0;
    double flops_per_img = 0, bytes_per_img = 0, weight_bytes = 0;
    bool fused_away = false;      // POOL steps whose work is done by the preceding conv's epilogue
    int head_step = -1;           // CONV: index of the HEAD step this layer feeds (candidate for the fused head), else -1
    bool feeds_head = false;      // CONV: its output is the fp32 head's input (stays fp32 in the 16-bit pipelines)
};

// What the plan is built from and routed with: the handle's settings and buffers, nothing else of it.
struct PlanInput {
    mi_unet_config cfg{};
    int algo = MI_UNET_CONV_DIRECT;   // resolved MI_UNET_CONV_* value
    bool fuse_pool = true;            // MIUNET_FUSE_POOL
    bool fuse_head = true;            // MIUNET_FUSE_HEAD
    float *weights = nullptr;         // device blob the HostWeights offsets point into
    float *cat[8]{}, *s0 = nullptr, *s1 = nullptr;      // concat buffers [Bm][h_i][w_i][2*ch_i] and the two scratch buffers ...
    size_t cat_floats[8]{}, s_floats = 0;               // ... with their capacities (plan_buffer_floats)
    // route_plan only
    Routing routing;
    bool guard_tripped = false;
    int wino4_min_wg = 256;
    const float *lut = nullptr;       // 256 floats: i / 255.0f
    float *ksplit = nullptr;          // split-K workspace
    size_t ksplit_bytes = 0;
};

// capacities of the activation buffers mi_unet_create allocates for cfg at max_batch (the transposed decoder's; the bilinear plan's
// tensors are smaller): the concat buffers of levels 0 .. levels - 1 and each of the two scratch buffers
void plan_buffer_floats(const mi_unet_config &cfg, size_t cat_floats[8], size_t &s_floats);

// (re)build the launch plan for micro-batch capacity cfg.max_batch; every tensor is checked against its buffer's capacity
int build_plan(const PlanInput &in, const HostWeights &hw, std::vector<Step> &plan);

// One step of the plan as this micro-batch launches it: its arguments (CONV / CONVT) and the route with the fusions granted.
struct Launch {
    ConvArgs a{};
    RouteChoice rc{ Route::FIRST, 0 };
    bool skip = false;            // done by a neighbour: pooling by its producer, the first layer by inc.c2, the head by the last conv
};

// Route every step for batch B
void route_plan(const PlanInput &in, const std::vector<Step> &plan, const uint8_t *d_imgs, int B, uint8_t *d_labels, float *d_logits,
                int lp_kind, std::vector<Launch> &out);

}  // namespace miunet
