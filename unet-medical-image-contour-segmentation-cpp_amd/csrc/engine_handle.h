// engine_handle.h -- struct mi_unet and what the units that implement include/mi_unet.h share: engine.cpp (create / destroy, weights,
// launch_plan, the u8 entry points), pipeline_raw.cpp, pipeline_tiled.cpp and debug.cpp, and through stage_common.h the host halves of
// the stages behind the network (texture_common.h for the three texture stages among them).  Internal to libmiunet.so.
#pragma once
#include <hip/hip_runtime.h>

#include <memory>
#include <string>
#include <utility>
#include <vector>

#include "../../include/mi_unet.h"
#include "copy_pool.h"
#include "engine_internal.h"
#include "graph_cache.h"
#include "kernels.h"
#include "plan.h"
#include "routing.h"

namespace miunet {

inline int fail(int code, const std::string &msg) { return engine_fail(code, msg); }

#define HIP_TRY(expr)                                                                                          \
    do {                                                                                                       \
        hipError_t e__ = (expr);                                                                               \
        if (e__ != hipSuccess)                                                                                 \
            return fail(MI_UNET_EHIP, std::string(#expr) + ": " + hipGetErrorString(e__));                    \
    } while (0)

// Owning device (hipMalloc) or pinned host (hipHostMalloc, hipHostMallocDefault) buffer of `n` elements: reset(n) frees what it
// held and allocates anew (0 = only free); the destructor frees.  The caller synchronises whatever may still use the old memory.
template <class T, bool PINNED>
struct Buffer {
    T *p = nullptr;
    Buffer() = default;
    Buffer(const Buffer &) = delete;
    Buffer &operator=(const Buffer &) = delete;
    ~Buffer() { (void)reset(0); }
    hipError_t reset(size_t n)
    {
        hipError_t e = !p ? hipSuccess : PINNED ? hipHostFree(p) : hipFree(p);
        p = nullptr;
        if (e == hipSuccess && n) e = PINNED ? hipHostMalloc(&p, n * sizeof(T), hipHostMallocDefault) : hipMalloc(&p, n * sizeof(T));
        return e;
    }
    T *get() const { return p; }
    operator T *() const { return p; }
};
template <class T> using DeviceBuf = Buffer<T, false>;
template <class T> using PinnedBuf = Buffer<T, true>;

inline size_t up256(size_t v) { return (v + 255) & ~(size_t)255; }      // the parts of a workspace start on 256-byte boundaries

// The parts of a workspace, one behind the other: take(bytes) is where the next part starts; `end` is the room taken so far.
struct Layout {
    size_t end = 0;
    size_t take(size_t bytes) { return std::exchange(end, end + up256(bytes)); }
};

// A stage's device buffer and its pinned staging, in bytes: grown on demand, owned by the handle, never shared with a clone.
struct Workspace {
    DeviceBuf<uint8_t> d;
    PinnedBuf<uint8_t> p;
    size_t dev_cap = 0, host_cap = 0;
    // at least dev_need / host_need bytes; whatever `s` still runs on the old memory completes before it is freed.  A failed allocation
    // leaves that side empty with a cap of 0
    int reserve(size_t dev_need, size_t host_need, hipStream_t s)
    {
        if (dev_need <= dev_cap && host_need <= host_cap) return MI_UNET_OK;
        HIP_TRY(hipStreamSynchronize(s));
        if (dev_need > dev_cap) {
            dev_cap = 0;
            HIP_TRY(d.reset(dev_need));
            dev_cap = dev_need;
        }
        if (host_need > host_cap) {
            host_cap = 0;
            HIP_TRY(p.reset(host_need));
            host_cap = host_need;
        }
        return MI_UNET_OK;
    }
};

struct Event {
    hipEvent_t e = nullptr;
    Event() = default;
    Event(Event &&o) noexcept : e(std::exchange(o.e, nullptr)) {}
    Event(const Event &) = delete;
    Event &operator=(const Event &) = delete;
    Event &operator=(Event &&o) noexcept { std::swap(e, o.e); return *this; }
    ~Event() { if (e) (void)hipEventDestroy(e); }
    hipError_t reset(unsigned flags = hipEventDefault)
    {
        if (e) (void)hipEventDestroy(e);
        e = nullptr;
        return hipEventCreateWithFlags(&e, flags);
    }
    hipEvent_t get() const { return e; }
    operator hipEvent_t() const { return e; }
};

// What the graph cache of a handle does with an executable that leaves it (engine.cpp): wait until nothing can still replay it,
// then hipGraphExecDestroy.
struct GraphRetire {
    mi_unet *h;
    void operator()(const GraphKey &key, hipGraphExec_t exec) const;
};

}  // namespace miunet

struct mi_unet {
    mi_unet_config cfg{};
    int ch[8]{};
    hipStream_t own_stream = nullptr;
    hipStream_t stream = nullptr;
    bool weights_loaded = false;
    int algo = MI_UNET_CONV_DIRECT; // resolved conv3x3 algorithm (MI_UNET_CONV_DIRECT / _WINOGRAD / _WINOGRAD16)
    bool fuse_pool = true;          // MIUNET_FUSE_POOL=0 keeps the stand-alone pooling kernel (A/B and parity checks)
    bool fuse_head = true;          // MIUNET_FUSE_HEAD=0 keeps the stand-alone head kernel
    int wino4_min_wg = 256;         // MIUNET_WINO4_MIN_WG: smallest grid the F(4x4,3x3) kernel takes (else F(2x2) + split-K)
    miunet::Routing routing;        // kernel-routing switches + CU count, resolved at create (kernels.h)
    // numeric guard of the default fp32 plan (engine_calibrate): F(4x4,3x3) is kept only if, for THIS weight set, a probe tile's
    // logits agree with the F(2x2,3x3) plan's within `guard_limit`; otherwise every layer runs F(2x2,3x3)
    bool wino4_guard_tripped = false;
    float guard_diff = -1.f, guard_limit = 5e-4f;
    std::string guard_text = "numeric guard: not run (no weights, or not the default fp32 plan)";
    // device memory
    // one blob: every packed tensor (single allocation -> one broadcast / one free).  Owned by `weights`, which clones of
    // this handle share (mi_unet_clone: the reference's engine is shared by its per-thread contexts, src/process.cpp:15, :69)
    std::shared_ptr<miunet::DeviceWeights> weights;
    // the assembly kernels' code objects on this handle's device (kernels.h): made by mi_unet_create for the fp32 Winograd plan unless
    // MIUNET_WINO4_ASM=0, shared with clones, unloaded with the last handle that holds it.  Null = this handle has none, and then
    // routing.wino4_asm is 0; asm_note (appended to guard_text) says why when they were wanted and could not be loaded
    std::shared_ptr<miunet::AsmKernels> asm_kernels;
    std::string asm_note;
    float *d_weights = nullptr;     // = weights->d
    size_t weight_floats = 0;
    miunet::DeviceBuf<float> d_lut;         // 256 floats: i / 255.0f
    miunet::DeviceBuf<float> d_cat[8];      // concat buffers [Bm][h_i][w_i][2*ch_i]
    miunet::DeviceBuf<float> d_s0, d_s1;
    size_t cat_floats[8]{}, s_floats = 0;   // their sizes (build_plan checks every step's tensors against them)
    miunet::DeviceBuf<uint8_t> d_img;       // staging for the host-buffer entry point
    miunet::DeviceBuf<uint8_t> d_labels;
    miunet::DeviceBuf<float> d_logits;
    // RAW16 staging for mi_unet_infer_raw16: a ring of (pinned host, device) buffer pairs, grown on demand, so the host copy
    // of image i+1 into its pinned buffer overlaps the PCIe transfer and the preprocessing kernels of image i
    static constexpr int RAW_RING = 3;
    miunet::DeviceBuf<uint16_t> d_raw[RAW_RING];
    miunet::PinnedBuf<uint16_t> h_raw[RAW_RING];
    miunet::Event raw_done[RAW_RING];       // the slot's transfer and kernels have completed
    bool raw_busy[RAW_RING] = {};
    size_t raw_cap = 0;             // samples per slot
    // one (lo, hi) slot of two u32 per plane of the running RAW-in call ([B * in_ch][2], tiled: [in_ch][2]; grown on demand):
    // written by the min/max or the window selection of the plane, read by its resample / normalise launch, downloaded once at the
    // end of the call into h_win for mi_unet_last_windows
    miunet::DeviceBuf<unsigned> d_mnmx;
    miunet::PinnedBuf<unsigned> h_win;
    size_t win_cap = 0;                     // slots of the two above
    // mi_unet_set_window; d_win_ws = zeroed-per-use scratch of launch_window_select_u16, one slot per plane of a micro-batch
    mi_unet_window window{ MI_UNET_WINDOW_MINMAX, 0, 0, 0, 65535 };
    miunet::DeviceBuf<uint8_t> d_win_ws;
    size_t win_ws_slots = 0;
    std::vector<int> win_src;               // per plane of the call: the plane whose slot holds its window (a pointer passed in_ch times)
    std::vector<int32_t> last_win;          // mi_unet_last_windows: (lo, hi) per plane of the last completed call
    bool last_win_valid = false;
    miunet::DeviceBuf<float> d_ksplit;      // split-K slabs of the Winograd kernel (small batches / deep levels only)
    size_t ksplit_bytes = 0;
    miunet::DeviceBuf<int> d_cont;          // contour outputs of mi_unet_extract_contours (grown on demand)
    miunet::PinnedBuf<int> h_cont;          // pinned mirror: one async D2H, then only the points that exist are copied to the caller
    size_t cont_cap = 0;            // ints
    // mi_unet_set_measure.  d_regions = the accumulators and the output of one micro-batch, [planes][cap] structs and
    // behind them [planes] counts; h_regions = its pinned mirrors, one per parity of the RAW pipeline; grown on demand
    // (grow_region_buffers).  last_regions / last_region_counts: the report of the last contour-returning call, all its planes.
    mi_unet_measure measure{ 0, 0 };
    miunet::DeviceBuf<uint8_t> d_regions;
    miunet::PinnedBuf<uint8_t> h_regions[2];
    size_t regions_cap = 0;         // bytes of each of the three
    std::vector<mi_unet_region> last_regions;
    std::vector<int32_t> last_region_counts;
    int last_region_planes = 0, last_region_cap = 0;
    bool last_regions_valid = false;
    // The workspaces of the stages behind the network, one per stage: the device side holds one call's inputs,
    // results and kernel scratch, the pinned side the staging of what crosses the bus.  The stage's entry point (csrc/<stage>.cpp) lays
    // its workspace out and grows it; no other stage, and no clone, touches it.
    // mi_unet_score_labels and mi_unet_score_volume: both maps, the scores, the kernels' workspace; pinned: the maps and the results.
    // Either call ends with a host synchronisation, so the two stages take turns on it
    miunet::Workspace ws_score;
    miunet::Workspace ws_volume;       // mi_unet_volume_components: the volume, out, ids, the table, the counts, the kernels' workspace
    miunet::Workspace ws_vclean;       // mi_unet_volume_clean: the volume, out, the counts, the kernels' workspace
    miunet::Workspace ws_vmesh;        // mi_unet_volume_mesh: the volume, the counts, the kernels' workspace
    miunet::Workspace ws_vmesh_out;    // ... the kept vertices and quads of one plane, sized by its counts
    miunet::Workspace ws_vms;          // mi_unet_volume_measure: ids, intensity, the table and the per-component arrays
    miunet::Workspace ws_vms_pts;      // ... the run ends of the searched components and the work list of the pair search, sized once the ends are counted
    miunet::Workspace ws_vsp;          // mi_unet_volume_spatial: ids, intensity, the table, the per-component arrays, the ball's rows, the row prefix sums
    miunet::Workspace ws_vsp_pts;      // ... the candidates, their ranks, the points of the searched components, both work lists and the slots, sized once the voxels are counted
    miunet::Workspace ws_vmt;          // mi_unet_volume_match: the results (side tables, `found`, pairs), the row offsets, the contingency table, both id stacks
    miunet::Workspace ws_vtx;          // mi_unet_volume_texture: the keys (ids in place), the intensity, the ranges, the table, the histograms, both co-occurrence tables
    miunet::Workspace ws_vzn;          // mi_unet_volume_zones: the results (table, found, both run tables, the zone list), the keys (ids in place), the intensity, the ranges, the forest
    miunet::Workspace ws_vnb;          // mi_unet_volume_nbhood: the results (table, the tables asked for), the keys (ids in place), the intensity, the ranges, the forest, both distance stacks
    miunet::Workspace ws_vsplit;       // mi_unet_volume_split: the volume, ids, the table, the info, the plane results, the rounds' activity, the kernels' workspace
    miunet::Workspace ws_vskel;        // mi_unet_volume_skeleton: the ids (the state, the skeleton), r2, the table, the pass state, the kernels' workspace
    miunet::Workspace ws_vbranch;      // mi_unet_volume_branches: the ids (the state), r2, the map, both tables, the per-id table, the round's words, the kernels' workspace
    miunet::Workspace ws_volume_interp; // mi_unet_volume_interp: the masks, out, the counts, both intensity stacks, the kernels' workspace
    // RAW-in entry points: a second stream uploads and preprocesses micro-batch k+1 into the other tile buffer while the
    // network of micro-batch k runs (d_img / d_img2 alternate)
    hipStream_t pre_stream = nullptr;
    miunet::DeviceBuf<uint8_t> d_img2;
    miunet::Event tile_ready[2];
    // stage timing of the last RAW-in call (mi_unet_last_stage_ms): event pairs per micro-batch, summed
    miunet::Event stage_ev[2][5], out_done[2];
    miunet::Event pre_ev[3][2];             // three pairs: micro-batch k + 2 is staged before k's times are read
    miunet::PinnedBuf<uint8_t> h_labels2;   // second pinned label buffer (infer): micro-batch k + 1 downloads while the host still copies k out
    // third stream of the RAW-in entry points: the tail (enqueue_tail) and the downloads of micro-batch k run here while the
    // engine's stream already works on the network of k + 1; own workspace (the network's scratch buffers, which the
    // single-stage entry points borrow, are in use by then), second label buffer
    hipStream_t tail_stream = nullptr;
    hipStream_t dl_stream = nullptr;          // tile downloads: behind the network of k, beside its tail and the upload of k + 1
    miunet::Event tiles_done[2];
    miunet::DeviceBuf<uint8_t> d_tail_ws;
    size_t tail_ws_bytes = 0;
    miunet::DeviceBuf<uint8_t> d_labels2;
    miunet::Event net_done[2], tail_ev[2][4];
    std::unique_ptr<miunet::CopyPool> copy_pool;   // helpers of the pageable -> pinned staging copy (created on first use)
    miunet::PinnedBuf<uint8_t> h_tiles[2];  // pinned mirrors of the tile buffers (a D2H into the caller's pageable memory would block the host)
    float stage_ms[MI_UNET_N_STAGES] = {};
    // tiled entry points (mi_unet_infer_tiled_*): the full-size image, its label map, logits and u16 planes stay
    // on the device for the whole call.  Grown on demand (ensure_tiled_buffers), owned by this handle, never shared with a clone.
    struct Tiled {
        miunet::DeviceBuf<uint8_t> d_img, d_labels;                                  // u8 [H][W][in_ch] (+ slack to a dword), [H][W]
        miunet::PinnedBuf<uint8_t> h_img, h_out;                                     // pinned mirrors of d_img and of d_labels
        size_t px_cap = 0;                                                   // pixels the four above hold
        miunet::DeviceBuf<float> d_logits;
        size_t logit_cap = 0;                                                // pixels
        miunet::DeviceBuf<uint16_t> d_raw;                                           // in_ch planes of u16 [H][W], device ...
        miunet::PinnedBuf<uint16_t> h_raw;                                           // ... and pinned
        size_t raw_cap = 0;                                                  // pixels per plane
        std::vector<miunet::Event> ev;                                               // stage boundaries of the last call
        miunet::DeviceBuf<uint8_t> d_multi;                                          // the segment forms: [K][H][W] masks / pictures ...
        miunet::PinnedBuf<uint8_t> h_multi;                                          // ... and their pinned mirror
        size_t multi_cap = 0;                                                // bytes
        miunet::DeviceBuf<float> d_acc;                                              // blending: fp32 accumulator [classes][H][W]
        size_t acc_cap = 0;                                                  // pixels
    } tiled;
    // mi_unet_set_tile_blend: how the tiled entry points combine overlapping tiles; d_blend_w = the weight tables of the tile height
    // and width (height + width floats), uploaded when the setting changes
    mi_unet_tile_blend blend{ MI_UNET_BLEND_OWNER, 0.125f, 0 };
    miunet::DeviceBuf<float> d_blend_w;
    // mi_unet_set_targets: what the _multi entry points segment.  d_multi / h_multi hold the [B][K][H][W] planes of every segment call
    // (masks, then their 0 / 255 pictures in place; K = 1 without _multi) and the pinned mirrors of two micro-batches in flight;
    // grown on demand (ensure_multi_buffers)
    mi_unet_target targets[MI_UNET_MAX_TARGETS] = { { 2, 0.06f } };
    int n_targets = 1;
    miunet::DeviceBuf<uint8_t> d_multi;
    miunet::PinnedBuf<uint8_t> h_multi[2];
    size_t multi_cap = 0;           // bytes of each of the three
    // mi_unet_set_morph: one entry for every target of a _multi call, or one per target
    mi_unet_morph morph[MI_UNET_MAX_TARGETS] = { { MI_UNET_MORPH_RECT, 1, 0 } };
    int n_morph = 1;
    // pinned host staging (the reference used pageable std::vector, src/process.cpp:138,152)
    miunet::PinnedBuf<uint8_t> h_img;
    miunet::PinnedBuf<uint8_t> h_labels;
    std::vector<miunet::Step> plan;
    // hipGraph replay of the forward pass (the reference replays a captured CUDA graph per image, src/process.cpp:99-105,
    // :147): one captured graph per (stream, buffers, batch) key; the first call of a key runs eagerly.  graph_cache.h holds the
    // policy (64 entries, first in first out); an executable that leaves the cache goes through GraphRetire, which waits for the
    // work that may still replay it.  left_streams: one event per caller's stream the handle was switched away from while the
    // cache held an executable captured on it, recorded on that stream at the switch (mi_unet_set_stream) -- behind everything the
    // handle ever enqueued there, and all GraphRetire needs of a stream that may be gone by the time its entries are evicted.
    static constexpr size_t GRAPH_CACHE_ENTRIES = 64;
    struct LeftStream { hipStream_t stream; miunet::Event done; };
    std::vector<LeftStream> left_streams;
    using GraphCache = miunet::GraphCache<hipGraphExec_t, miunet::GraphRetire>;
    GraphCache graphs{ GRAPH_CACHE_ENTRIES, miunet::GraphRetire{ this } };     // (mi_unet_destroy clears it while the streams live)
    bool use_graph = true;          // MIUNET_GRAPH=0 disables
    // the RAW-in entry points' switches (pipeline_raw.cpp), parsed at create like the ones above and copied by mi_unet_clone
    int copy_threads = 4;           // MIUNET_COPY_THREADS (1..16): threads of a large host copy; 1 = plain memcpy
    std::vector<int> raw_split{ -1 };   // MIUNET_RAW_SPLIT: { 0 } whole chunks only, { a, b, ... } cuts of the first chunk, { -1 } the default cut
    bool raw_trace = false;         // MIUNET_RAW_TRACE=1: host-side timeline of every RAW-in call on stderr
    bool postprocess = false;       // mi_unet_set_postprocess: label maps -> postprocess_mask output before they leave the device
    // profiling: one event pair per launch, recorded on the launch stream and only read back (synchronised) in
    // mi_unet_get_kernel_stats, so the launches themselves never wait on the host
    bool profiling = false;
    std::vector<mi_unet_kernel_stat> stats;
    std::vector<miunet::Event> ev_pool;
    size_t ev_used = 0;
    miunet::Event tev0, tev1;
    // mi_unet_debug_capture: stop launch_plan after step `layer` and hand its operands of image `img` to the host
    struct Tap {
        int layer = -1, img = 0;
        float *in = nullptr, *out = nullptr, *pooled = nullptr;
        uint8_t *labels = nullptr;
        mi_unet_layer_info *info = nullptr;
        bool hit = false;
    } tap;
};

namespace miunet {

// ---- engine.cpp
int check_handle(mi_unet *h, bool need_weights);
PlanInput plan_input(const mi_unet *h);                 // the handle's settings and buffers as build_plan / route_plan take them
int launch_plan(mi_unet *h, const uint8_t *d_imgs, int B, uint8_t *d_labels, float *d_logits);
int run_microbatch(mi_unet *h, const uint8_t *d_imgs, int B, uint8_t *d_labels, float *d_logits);   // graph replay of launch_plan
int infer_microbatch(mi_unet *h, const uint8_t *d_imgs, int B, uint8_t *d_labels, float *d_logits);  // ... + postprocess when set
hipError_t launch_route(Route r, const ConvArgs &a, const AsmKernels *k, hipStream_t s);   // k: for the CONV_WINO4A / _WINO4B rows
constexpr mi_unet_target kDefaultTarget{ 2, 0.06f };    // the reference's: class 2, 6 % of the image
TargetTable target_table(const mi_unet_target *targets, int n, int H, int W);   // `n` targets with min_area of an H x W image
TargetTable target_table(const mi_unet *h, int H, int W);   // ... the handle's, with its morphology (the _multi entry points)
constexpr mi_unet_morph kDefaultMorph{ MI_UNET_MORPH_RECT, 1, 0 };      // the reference's 3x3 open
// a _multi call begins: MI_UNET_ESTATE + message when the handle's morphology list (mi_unet_set_morph) fits neither every target nor each
int check_morph_list(const mi_unet *h, const char *fn);
void table_morph(TargetTable &t, const mi_unet_morph *m, int n);       // entry k % n of `m` for target k (n = 1 or t.K)
TargetTable default_targets(int H, int W);              // ... the reference's (every entry point without _multi, whatever the handle's setting)
// h->d_tail_ws of at least `ws_bytes`, h->d_multi / h->h_multi[0..1] of at least `plane_bytes` each (synchronises their users before they grow)
int ensure_tail_buffers(mi_unet *h, size_t ws_bytes, size_t plane_bytes);
int grow_events(std::vector<Event> &ev, size_t n);      // at least n timing events (never inside a capture)
// The contour arrays of `planes` masks (launch_extract_contours) as one run of ints -- xy, start, count -- from `base`: h->d_cont,
// or a half of its pinned mirror h->h_cont.
struct ContourLayout {
    int planes, cap_points, cap_contours;
    size_t ints() const { return (size_t)planes * ((size_t)cap_points * 2 + cap_contours + 1 + 1); }
    template <class T> T *xy(T *base) const { return base; }
    template <class T> T *start(T *base) const { return base + (size_t)planes * cap_points * 2; }
    template <class T> T *count(T *base) const { return start(base) + (size_t)planes * (cap_contours + 1); }
};
// contour outputs: device -> pinned mirror half (async on `s`) -> the caller's arrays (after the synchronise)
int grow_contour_buffers(mi_unet *h, const ContourLayout &cl);
int contours_to_pinned(mi_unet *h, const ContourLayout &cl, hipStream_t s, int half = 0);
void contours_to_caller(const mi_unet *h, const ContourLayout &cl, int32_t *xy, int32_t *start, int32_t *counts, int half = 0);
// The tail behind the argmax, enqueued on `s`: postprocess_mask of B label maps per target of `t` -> d_planes u8 [B][t.K][H][W] in
// {0, cls} (d_labels itself allowed when t.K == 1); with `cl` (cl->planes == B * t.K): -> their 0 / 255 pictures in place -> contours
// into h->d_cont.  `ws` holds both stages' workspaces for B * t.K planes (checked by the caller); `between` (or null) is recorded
// behind the postprocess, the boundary of the two stage times; `where` prefixes the message of a failed launch.  An empty table
// (t.K == 0, no cl) enqueues nothing but `between`.
// With `m` (the handle measures, cl given): the regions of the cl->planes masks behind the contours, from m->d_tiles (the u8
// [B][H][W][in_ch] the planes' images were read from), into h->d_regions and on into the pinned mirror m->half, all on `s`.
struct MeasureArgs { const uint8_t *d_tiles; int half; };
int enqueue_tail(mi_unet *h, const uint8_t *d_labels, int B, int H, int W, const TargetTable &t, uint8_t *d_planes, void *ws,
                 const ContourLayout *cl, hipEvent_t between, hipStream_t s, const std::string &where = std::string(),
                 const MeasureArgs *m = nullptr);
// ---- measure.cpp: region measurement (mi_unet_set_measure)
// The region arrays of `planes` masks as one run of bytes: [planes][cap] structs, then [planes] counts.
struct RegionLayout {
    int planes, cap;
    size_t bytes() const { return (size_t)planes * cap * sizeof(mi_unet_region) + (size_t)planes * sizeof(int32_t); }
    mi_unet_region *regions(uint8_t *base) const { return reinterpret_cast<mi_unet_region *>(base); }
    const mi_unet_region *regions(const uint8_t *base) const { return reinterpret_cast<const mi_unet_region *>(base); }
    int32_t *counts(uint8_t *base) const { return reinterpret_cast<int32_t *>(base + (size_t)planes * cap * sizeof(mi_unet_region)); }
    const int32_t *counts(const uint8_t *base) const { return reinterpret_cast<const int32_t *>(base + (size_t)planes * cap * sizeof(mi_unet_region)); }
};
int check_measure_size(int H, int W, const std::string &fn);   // MI_UNET_EARG where a moment sum could pass 2^62 (include/mi_unet.h)
int grow_region_buffers(mi_unet *h, const RegionLayout &rl);   // nothing may be in flight on them
// a contour-returning call begins: the report is invalid until the call has completed; measuring: room for `planes` planes
void begin_region_call(mi_unet *h, bool measuring, int planes, int cap);
// mirror `half` holds the planes [plane0, plane0 + rl.planes) of the running call (after the synchronise)
void regions_to_report(mi_unet *h, const RegionLayout &rl, int plane0, int half);
void finish_region_call(mi_unet *h);                           // the call has completed: the report is valid
// ---- window.cpp: the intensity window of the RAW-in entry points
constexpr mi_unet_window kDefaultWindow{ MI_UNET_WINDOW_MINMAX, 0, 0, 0, 65535 };
int check_window(const mi_unet_window &w, const char *fn);   // MI_UNET_EARG + message for a setting mi_unet_set_window refuses
// before a RAW-in call enqueues anything: slots for `planes` windows, scratch for `scratch_planes` selections at once (PERCENTILE only),
// and the call's bookkeeping reset.  PERCENTILE refuses a plane of 2^32 samples or more (max_samples = the call's largest plane).
int begin_window_call(mi_unet *h, size_t planes, size_t scratch_planes, unsigned long long max_samples, const std::string &fn);
// min/max or selection of one plane into slot `slot` (scratch slot `ws_slot`) on `s`; FIXED enqueues nothing
hipError_t enqueue_window(mi_unet *h, const uint16_t *d_raw, size_t n, size_t slot, size_t ws_slot, hipStream_t s);
int enqueue_window_download(mi_unet *h, size_t planes, hipStream_t s);     // slots -> h_win (nothing for FIXED)
void finish_window_call(mi_unet *h, size_t planes);                        // after the download has completed: h_win -> last_win
// ---- pipeline_raw.cpp: large host copies on the handle's helper threads
void host_copy(mi_unet *h, void *dst, const void *src, size_t bytes);
// ---- debug.cpp: mi_unet_debug_capture's taps, called by launch_plan around the tapped step
int tap_input(mi_unet *h, const Step &st, const Launch &l, const uint8_t *d_imgs, int lp_kind);
int tap_output(mi_unet *h, const Step &st, const Launch &l, uint8_t *d_labels, float *d_logits, int lp_kind);

}  // namespace miunet
