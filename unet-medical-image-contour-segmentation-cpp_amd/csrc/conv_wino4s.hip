// conv_wino4s.hip -- Winograd F(4x4,3x3) for the layers with at most 64 output channels per workgroup, built so that TWO
// workgroups share a compute unit.  fp32 arithmetic on v_mfma_f32_16x16x4_f32, gfx950 only.
//
// Why a second kernel.  The one-block variant of conv_wino4.hip (NB = 1) holds one 144 KB workgroup per CU and threads the
// forward transform, the raw-patch DMA and the U ring between its MFMAs.  On the three top-level layers (inc.c2, up4.c1,
// up4.c2 + head: K = 4 or 8 chunks of 16 channels, 1-2 GiB of activations each) its matrix pipe is only 37-46 % busy
// (rocprofv3 SQ_VALU_MFMA_BUSY_CYCLES, profiles/r02a_pmc_fp32.json): a tile spends about as long in its prologue, in the
// stalls of chunks that open new 128-byte lines, and in its epilogue as in its MFMAs, and with one wave per SIMD nothing
// else can issue meanwhile.  On gfx950 the fp32 MFMA never co-executes with VALU work anyway (SQ_VALU_MFMA_COEXEC_CYCLES
// = 0 on every fp32 kernel of this library), so interleaving buys latency hiding only -- and a second resident workgroup
// buys the same, for every kind of stall at once, with much simpler code.
//
// Shape.  Workgroup = 4 waves = a 16x16 block of output pixels (16 tiles of 4x4) x 64 output channels; wave w owns 16
// channels for all 36 positions: 36 accumulators of 4 registers = 144, the whole kernel inside 256 registers
// (__launch_bounds__(256, 2)).  LDS = ONE V image [36][16 tiles][16] (36,864 B) + ONE raw patch image
// [18 rows][20 slots][16 channels] (23,552 B) = 60,416 B, twice per CU.  A K-chunk of 16 input channels is three phases:
//      wait for the chunk's raw patch (LDS-DMA, vmcnt) | barrier | forward transform raw -> V | barrier |
//      144 MFMAs per wave, with the DMA of the NEXT chunk's patch and the U ring (16-byte buffer loads, three positions
//      ahead) issued between them
// Single buffers cost two barriers per chunk and serialise transform and MFMAs inside a workgroup; the co-resident
// workgroup runs its MFMAs meanwhile.  Everything else -- the slot-permuted raw image, the row-split forward transform,
// the in-lane inverse transform, the free bias at position (1,1), buffer stores, fused pooling, the fused 1x1 head -- is
// the arithmetic of conv_wino4.hip, and since both kernels take it from wino4_common.h it is one definition.  Their results
// are still not promised bit for bit: hipcc contracts multiply-adds per instruction stream, and the two schedules differ
// (test_conv3x3_wino4s_two_workgroups_per_cu allows 2e-5 between them).
#include <cstdlib>

#include "kernel_common.h"
#include "routing.h"
#include "wino4_common.h"

namespace miunet {

struct W4S {
    static constexpr size_t LDS_BYTES = sizeof(float) * (W4::VBUF + W4::RAW_FLOATS);          // 60,416
    static constexpr size_t LDS_BYTES_HEAD = head_lds_bytes(64);                              // the head tile (larger than V + raw) + its weights
    static constexpr int FIRST_WIN = 20;                    // fused first layer: the normalised (16 + 4)^2 window of the image behind V + raw
    static constexpr int FIRST_WMAX = WINO4S_FIRST_WMAX;                  // ... and the first layer's weights [9][Cin] + shift [Cin] (Cin <= 64: no long-lived registers)
    static constexpr size_t LDS_BYTES_FIRST = LDS_BYTES + sizeof(float) * (FIRST_WIN * FIRST_WIN + 10 * FIRST_WMAX);
    static_assert(LDS_BYTES <= sizeof(float) * 256 * W4::HEAD_ROW, "the head launch's allocation must cover the K loop's V + raw images");
};

// UD = U prefetch distance in positions (36 % UD == 0).  The ring is carried across the chunk boundary: its first UD loads of
// chunk c+1 fly during the barriers and the transform of that chunk, at 4 UD live registers there.  Round 3 priced the K loop's
// operand streams with timing-only builds (EXP below, profiles/r03_ab_wino4s_k_loop.txt): never refilling the U ring makes these
// layers 15-25 % faster, no patch DMA inside the loop 12-20 % -- a ring of three positions is 384 cycles of lead against an L2
// round trip, and a wave's vmcnt counts its loads in order.  UD = 6 is the deepest ring that compiles without spills next to the
// transform's temporaries since the branch-free role code (round 2: three): these layers -3 ... -10 %, the step 17.19 -> 16.89 ms
// same card.  Nine and twelve positions fit only with the two-row waves building their rows one after the other (24 fewer live
// registers, the patch column read twice): slower than six with the one-pass transform.  (Round 2: refilling a deeper ring AFTER the
// transform instead measured 15-40 % slower -- spills, and the refill's latency at the head of every MFMA phase.)
// EXP != 0: timing-only experiment builds (MIUNET_W4S_EXP; results are WRONG, never routed by default; switch the numeric guard off,
// MIUNET_WINO4_GUARD=0, or it sends the whole plan to F(2x2)): 1 = the U ring is never refilled, 2 = no raw-patch DMA inside the K
// loop, 3 = both
// LATE: the next chunk's raw patch is requested in the LAST six positions of the MFMA phase instead of at every fourth position from
// the first on: a wave's vmcnt is in order, so every U fragment younger than a patch request waits for HBM with it; requested late,
// the patch's latency falls into the wait in front of the next transform, which the co-resident workgroup's MFMAs cover
// (inc.c2 -2 %, up4.c1 -2.8 %, the others unchanged: profiles/r03_ab_wino4s_k_loop.txt).
// FIRST: the layer's input is the network's FIRST layer, computed here (ConvArgs::first_img): instead of the LDS-DMA of a raw chunk,
// every thread builds its 16-byte piece of the patch image -- the same (slot, channel quad) piece the DMA would have written --
// from a 20x20 window of the u8 image that the workgroup normalises once: acc = sum over the nine taps (raster order, fma chain from
// 0), + shift, ReLU: bit for bit what conv3x3_first_kernel stores, zero where the patch leaves the image (this layer's padding).
template <bool HEAD, int UD, int EXP = 0, bool LATE = true, bool FIRST = false>
__global__ __launch_bounds__(256, 2) void conv3x3_wino4s_f32(const ConvArgs a, const int tiles_x, const int tiles_y,
                                                             const int m_tiles, const int nwg)
{
    constexpr int VROW = W4::VROW, VPOS = W4::VPOS;
    static_assert(36 % UD == 0, "ring depth must divide the position count");
    extern __shared__ __attribute__((aligned(16))) float lds[];
    float *const Vs = lds;                    // [36][16][VROW]
    float *const Raw = lds + W4::VBUF;        // [18 rows][20 slots][16]
    float *const Win = Raw + W4::RAW_FLOATS;  // FIRST: [20][20] normalised image window, origin (by0 - 2, bx0 - 2)
    float *const Wf = Win + W4S::FIRST_WIN * W4S::FIRST_WIN;      // FIRST: [9][Cin] weights, then [Cin] shifts

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int j16 = lane & 15, kq = lane >> 4;

    // ---- this workgroup's tile (bijective XCD remap: the workgroups of one XCD walk neighbouring tiles, kernel_common.h)
    int L = xcd_remap(blockIdx.x, nwg);
    const int n_tile = L / m_tiles;
    int m = L - n_tile * m_tiles;
    const int tx = m % tiles_x; m /= tiles_x;
    const int ty = m % tiles_y;
    const int b = m / tiles_y;
    const int bx0 = tx * 16, by0 = ty * 16;
    const int ncol0 = n_tile * 64 + 16 * wave + j16;
    const unsigned u_voff = (unsigned)(ncol0 * WINO4_KC + 4 * kq) * 4;
    const __amdgpu_buffer_rsrc_t in_rsrc = __builtin_amdgcn_make_buffer_rsrc(
        const_cast<float *>(a.in + (size_t)b * a.H * a.W * a.ldc), 0, a.H * a.W * a.ldc * 4, 0x00020000);

    // ---- raw halo patch of one 16-channel chunk: global -> LDS by DMA (4 lanes = one pixel's 64 bytes; zero padding, channels
    // past Cin and dead slots through the buffer range check: voffset 0xFFFFFFFF reads zeros)
    unsigned raw_voff[W4::RAW_ITERS];
#pragma unroll
    for (int s = 0; s < W4::RAW_ITERS; ++s) raw_voff[s] = w4_raw_slot(a, by0, bx0, wave + 4 * s, lane).voff;
    auto first_patch = [&](int chunk) {                        // FIRST: this thread's pieces of a chunk's patch, computed
        const int cq = chunk * WINO4_KC + 4 * (lane & 3);
        const float *wq = Wf + cq;                             // tap t: wq[t * Cin .. + 3]; the shifts behind the ninth tap
#pragma unroll 1                                               // a real loop: unrolled, hipcc hoists 6 x 18 LDS reads and spills accumulators
        for (int s = 0; s < W4::RAW_ITERS; ++s) {
            if (wave + 4 * s >= W4::RAW_LOADS) break;
            // (w4_raw_slot's map written out: called from this real loop it costs inc.c2 0.03 ms of 1.13, EXPERIMENTS R5.20)
            const int g = (wave + 4 * s) * 16 + (lane >> 2);
            const int py = g / W4::RAW_ROW, sl = g - py * W4::RAW_ROW;
            const int px = 4 * (sl % 5) + sl / 5;
            const int gy = by0 - 1 + py, gx = bx0 - 1 + px;
            const bool inb = g < W4::RAW_SLOTS && px < 18 && gy >= 0 && gy < a.H && gx >= 0 && gx < a.W;
            f32x4 r = f32x4{ 0.f, 0.f, 0.f, 0.f };
            if (inb) {
                f32x4 acc = f32x4{ 0.f, 0.f, 0.f, 0.f };
                const float *wp = Win + py * W4S::FIRST_WIN + px;      // tap (dy, dx) of patch pixel (py, px): window (py + dy, px + dx)
#pragma unroll
                for (int t = 0; t < 9; ++t) acc += wp[(t / 3) * W4S::FIRST_WIN + t % 3] * *reinterpret_cast<const f32x4 *>(wq + t * a.Cin);
                const f32x4 a4 = acc + *reinterpret_cast<const f32x4 *>(wq + 9 * a.Cin);
                r.x = a4.x > 0.f ? a4.x : 0.f; r.y = a4.y > 0.f ? a4.y : 0.f; r.z = a4.z > 0.f ? a4.z : 0.f; r.w = a4.w > 0.f ? a4.w : 0.f;
            }
            *reinterpret_cast<f32x4 *>(Raw + (size_t)g * WINO4_KC + 4 * (lane & 3)) = r;
        }
    };
    auto dma_one = [&](int chunk, int s) {                     // the wave's s-th load (load wave + 4s) of a chunk's patch
        raw_dma_one(in_rsrc, Raw, chunk, wave + 4 * s, raw_voff[s], raw_chunk_ok(a.Cin, chunk, lane));
    };

    // ---- forward transform V = B^T d B of one chunk: the steps of wino4_common.h back to back, wave w in role w
    const W4Role role = w4_role(wave, lane);
    auto transform = [&]() {
        f32x4 cR[2][6];                       // rows of B^T d (row b only on the two-row waves)
#pragma unroll
        for (int k = 0; k < 6; ++k) {
            f32x4 d[4];
            w4_col_load(Raw + role.rd_off, role.rstride, k, d);
            w4_col(role.two, role.c_alpha, role.c_beta, d, cR[0][k], cR[1][k]);
        }
#pragma unroll
        for (int row = 0; row < 2; ++row) {
            if (row == 1 && !role.two) break;
            w4_row_pass(cR[row], Vs + role.wr_off + row * 6 * VPOS);
        }
    };

    // ---- MFMA role: wave w, channels n0 + 16 w .. + 15, all 36 positions
    const unsigned u_pos_bytes = (unsigned)a.CoutPad * WINO4_KC * 4;
    const int nchunks = (a.Cin + WINO4_KC - 1) / WINO4_KC;
    const __amdgpu_buffer_rsrc_t u_rsrc = w4_u_rsrc(a);
    auto u_load = [&](int chunk, int p) { return w4_u_load(u_rsrc, u_voff, u_pos_bytes, chunk, p); };
    const float *const v_rd = Vs + j16 * VROW + 4 * (kq ^ v_swz(j16));                       // + pos*VPOS

    // the loads that open the tile: the raw patch of chunk 0 straight into LDS, then the U ring
    if constexpr (FIRST) {
        const uint8_t *imgb = a.first_img + (size_t)b * a.H * a.W;
        for (int i = tid; i < W4S::FIRST_WIN * W4S::FIRST_WIN; i += 256) {
            const int y = i / W4S::FIRST_WIN, x = i - y * W4S::FIRST_WIN, gy = by0 - 2 + y, gx = bx0 - 2 + x;
            Win[i] = (gy >= 0 && gy < a.H && gx >= 0 && gx < a.W) ? a.first_lut[imgb[(size_t)gy * a.W + gx]] : 0.f;
        }
        for (int i = tid; i < 10 * a.Cin; i += 256) Wf[i] = i < 9 * a.Cin ? a.first_w[i] : a.first_shift[i - 9 * a.Cin];
    } else {
#pragma unroll
        for (int s = 0; s < W4::RAW_ITERS; ++s) dma_one(0, s);
    }
    f32x4 u[UD];
#pragma unroll
    for (int p = 0; p < UD; ++p) u[p] = u_load(0, p);

    f32x4 acc[36];
#pragma unroll
    for (int p = 0; p < 36; ++p) {
        const float init = w4_acc_init(a, p, ncol0);
#pragma unroll
        for (int r = 0; r < 4; ++r) acc[p][r] = init;
    }

    int chunk = 0;                            // at least one chunk: a do-while has no zero-trip path to merge accumulators with
    do {
        // the patch DMA of this chunk is older than the UD youngest loads (the U ring): wait for everything but those
        constexpr int LEFT = LATE ? 0 : UD;           // (late patch requests interleave with the ring's refills: wait for everything)
        if constexpr (FIRST) {
            if (chunk == 0) __syncthreads();  // the image window is complete
            first_patch(chunk);               // (the raw image is free: its last reader, the transform, is behind a barrier)
        } else {
            __builtin_amdgcn_s_waitcnt(0x0F70 | (LEFT & 15) | ((LEFT >> 4) << 14));
        }
        __syncthreads();                      // every wave's part of the patch has landed; nobody reads V any more
        transform();
        __syncthreads();                      // V complete, the raw image is free again
        const bool more = chunk + 1 < nchunks;
        const int nxt = more ? chunk + 1 : chunk;                          // the last chunk prefetches itself: straight-line code
        f32x4 av = *reinterpret_cast<const f32x4 *>(v_rd);
#pragma unroll
        for (int p = 0; p < 36; ++p) {
            f32x4 avn = av;
            if (p + 1 < 36) avn = *reinterpret_cast<const f32x4 *>(v_rd + (p + 1) * VPOS);   // V fragment one position ahead
            // one DMA load every fourth position, not a burst: 16 line misses at a time keep the VMEM queue moving
            if (!FIRST && more && !(EXP & 2)) {   // one DMA load per position (16 line misses at a time keep the VMEM queue moving)
                if (!LATE && p % 4 == 0 && p / 4 < W4::RAW_ITERS) dma_one(chunk + 1, p / 4);
                if (LATE && p >= 36 - W4::RAW_ITERS) dma_one(chunk + 1, p - (36 - W4::RAW_ITERS));
            }
            __builtin_amdgcn_sched_barrier(0);
            const f32x4 bv = u[p % UD];
#pragma unroll
            for (int s = 0; s < 4; ++s) acc[p] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[s], bv[s], acc[p], 0, 0, 0);
            const int pn = p + UD;                                                              // refill the ring slot
            if constexpr (!(EXP & 1)) u[p % UD] = u_load(pn < 36 ? chunk : nxt, pn % 36);
            av = avn;
            __builtin_amdgcn_sched_barrier(0);
        }
    } while (++chunk < nchunks);

    // ---- epilogue (w4_epilogue, wino4_common.h): inverse transform in-lane, ReLU, stores, pooled maxima or the head's tile.
    // (Swapping the MFMA operand roles would give every lane four consecutive CHANNELS of one tile and so 16-byte stores,
    // a quarter of the store instructions: measured 2-4 % slower on these layers -- the stores are bound by the 64-byte
    // segments they scatter, not by their count.)
    const int Hp = a.H >> 1, Wp = a.W >> 1;
    const bool do_pool = a.pool_out != nullptr;
    const __amdgpu_buffer_rsrc_t out_rsrc = __builtin_amdgcn_make_buffer_rsrc(a.out + (size_t)b * a.H * a.W * a.ldo, 0, a.H * a.W * a.ldo * 4, 0x00020000);
    const __amdgpu_buffer_rsrc_t pool_rsrc = __builtin_amdgcn_make_buffer_rsrc(
        do_pool ? a.pool_out + (size_t)b * Hp * Wp * a.pool_ld : a.out, 0, do_pool ? Hp * Wp * a.pool_ld * 4 : 0, 0x00020000);
    W4Out o;
    o.ld = a.ldo; o.co_off = a.co_off; o.by0 = by0; o.bx0 = bx0; o.relu_lo = a.relu ? 0.f : -__builtin_inff(); o.do_pool = do_pool;
    if constexpr (HEAD) __syncthreads();      // the head tile overwrites V: every wave must be past its last MFMA phase
    w4_epilogue<HEAD, ST_AUX, 1>(a, o, out_rsrc, pool_rsrc, acc, ncol0, ncol0 & 63, kq, lds);
    if constexpr (HEAD) fused_head_tile<64, 16>(a, lds, tid, b, by0, bx0);     // the four waves hold 16 channels each: the tile crossed LDS
}

template <bool HEAD>
static hipError_t launch_wino4s_cfg(const ConvArgs &a, hipStream_t s)
{
    const int tiles_x = (a.W + 15) / 16, tiles_y = (a.H + 15) / 16;
    const int m_tiles = tiles_x * tiles_y * a.B;
    const int n_tiles = (a.Cout + 63) / 64;
    const int nwg = m_tiles * n_tiles;
    size_t lds_bytes = HEAD ? W4S::LDS_BYTES_HEAD : W4S::LDS_BYTES;
    const bool first = a.first_img != nullptr;
    if (first) {
        if (HEAD || !conv3x3_wino4s_can_fuse_first(a, 1)) return hipErrorInvalidValue;
        lds_bytes = W4S::LDS_BYTES_FIRST;
    }
    // experiment switch: MIUNET_WINO4S_ONE_WG=1 asks for more than half a CU's LDS, so only ONE workgroup is
    // resident per CU -- the same kernel, same instructions, without its co-resident partner.  What that costs is what any
    // one-workgroup-per-CU re-tiling of these layers (a 32-tile block on v_mfma_f32_32x32x2_f32 needs 56 % of the register
    // file for its accumulators alone) would first have to win back.
#ifdef MIUNET_EXPERIMENTS                              // lab build only (libmiunet_exp.so, tools/dev/ab*.sh): never in libmiunet.so
    static const bool one_wg = [] { const char *e = getenv("MIUNET_WINO4S_ONE_WG"); return e && e[0] == '1'; }();
    if (one_wg) lds_bytes = 96 * 1024;
    static const int exp = [] { const char *e = getenv("MIUNET_W4S_EXP"); return e ? atoi(e) : 0; }();        // timing-only builds (see the kernel)
    static const int ud = [] { const char *e = getenv("MIUNET_W4S_UD"); return e ? atoi(e) : 6; }();            // A/B: =3 round 2's ring and early patch requests, =60 ring of six with early requests
#endif
    auto launch = [&](auto kern) {
        if (hipError_t e = ensure_dynamic_lds(kern, lds_bytes); e != hipSuccess) return e;
        hipLaunchKernelGGL(kern, dim3(nwg), dim3(256), lds_bytes, s, a, tiles_x, tiles_y, m_tiles, nwg);
        return hipGetLastError();
    };
#ifdef MIUNET_EXPERIMENTS
    if (exp == 1) return launch(conv3x3_wino4s_f32<HEAD, 3, 1, false>);
    if (exp == 2) return launch(conv3x3_wino4s_f32<HEAD, 3, 2, false>);
    if (exp == 3) return launch(conv3x3_wino4s_f32<HEAD, 3, 3, false>);
    if (ud == 3) return launch(conv3x3_wino4s_f32<HEAD, 3, 0, false>);
    if (ud == 60) return launch(conv3x3_wino4s_f32<HEAD, 6, 0, false>);
#endif
    if constexpr (!HEAD) { if (first) return launch(conv3x3_wino4s_f32<false, 6, 0, true, true>); }
    return launch(conv3x3_wino4s_f32<HEAD, 6>);
}

// the fused first layer: one input channel, whole 16-channel chunks of its output (= this layer's input), no fused head
// Same contract as the one-block variant of launch_conv3x3_wino4 (a.wpk4 = U packed [Cin/16][36][CoutPad][16]); no split-K.
hipError_t launch_conv3x3_wino4s(const ConvArgs &a, hipStream_t s)
{
    if (a.wpk4 == nullptr || a.Cin % 4 || (a.first_img == nullptr && a.ldc % 4) || a.CoutPad % NPAD) return hipErrorInvalidValue;
    if (a.head_w != nullptr) {
        if (a.Cout > 64 || a.head_classes < 1 || a.head_classes > 4 || a.pool_out != nullptr || a.head_labels == nullptr)
            return hipErrorInvalidValue;
        return launch_wino4s_cfg<true>(a, s);
    }
    return launch_wino4s_cfg<false>(a, s);
}

}  // namespace miunet
