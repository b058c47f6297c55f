// wino4_common.h -- the arithmetic of the two Winograd F(4x4,3x3) kernels (conv_wino4.hip, conv_wino4s.hip), each piece once:
// the raw-patch slot map and its LDS-DMA load, the forward transform's steps, the U loads, the accumulators' initial value and
// the epilogue.  Each kernel keeps its schedule: where between its MFMAs, barriers and waits it calls them.  Two written-out
// copies remain, because the call measured slower (docs/EXPERIMENTS.md R5.20): the transform's steps as the numbered pieces of
// conv_wino4.hip, and the slot map inside conv_wino4s.hip's first_patch.  A change here is made there too.  Internal.
// The helpers are plain inline functions, like the kernels' own lambdas: forcing them in early changes the register allocation
// of kernels that live at 255 of 256 VGPRs (accumulators copied through v_mov_b64).  They take ConvArgs by value, as the kernels
// hold it: through a reference the same bodies come out 20 - 60 instructions longer per kernel.
#pragma once
#include <type_traits>

#include "kernel_common.h"

namespace miunet {

// a - b on packed pairs: hipcc scalarises a plain fsub of <4 x float> into four v_sub_f32; two v_pk_add_f32 with a negated
// operand do the same work in half the issue slots (the matrix pipe shares them)
typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
__device__ __forceinline__ f32x4 pk_sub(const f32x4 a, const f32x4 b)
{
    f32x2 lo, hi;
    asm("v_pk_add_f32 %0, %1, %2 neg_lo:[0,1] neg_hi:[0,1]" : "=v"(lo) : "v"(a.lo), "v"(b.lo));
    asm("v_pk_add_f32 %0, %1, %2 neg_lo:[0,1] neg_hi:[0,1]" : "=v"(hi) : "v"(a.hi), "v"(b.hi));
    return __builtin_shufflevector(lo, hi, 0, 1, 2, 3);
}

__device__ __forceinline__ f32x2 pk_sub2(const f32x2 a, const f32x2 b)
{
    f32x2 r;
    asm("v_pk_add_f32 %0, %1, %2 neg_lo:[0,1] neg_hi:[0,1]" : "=v"(r) : "v"(a), "v"(b));
    return r;
}


__device__ __forceinline__ int v_swz(int tile) { return 2 * ((tile >> 2) & 1); }

struct W4 {
    static constexpr int TMB = 16;                          // 4x4 output tiles per workgroup (4 wide x 4 tall)
    // V rows are 64 bytes, unpadded; the 16-byte channel quad q of tile t sits in slot q ^ v_swz(t).  The MFMA operand read has
    // lane = (tile lane & 15, quad lane >> 4), and gfx950 services a ds_read_b128 in groups of 16 lanes {0-3, 12-15, 20-27},
    // {4-11, 16-19, 28-31} (+ 32): a group holds tiles {0-3, 12-15} with one quad and {4-11} with the next, which 80-byte padded
    // rows (rounds 1-2: "5 t mod 16 is a bijection", true for 16 CONSECUTIVE lanes) serve with a 2-way conflict -- 8 LDS cycles
    // per read instead of 4 (tools/dev/lds_bank_model.py).  The transform's ds_write_b128 (lane = (tile lane >> 2, quad lane & 3):
    // eight consecutive lanes = two tiles = 128 contiguous bytes) is conflict-free either way.
    static constexpr int VROW = WINO4_KC;                   // floats per tile row of V
    static constexpr int VPOS = TMB * VROW;                 // floats per position
    static constexpr int VBUF = 36 * VPOS;                  // floats per V buffer
    static constexpr int RAWPIX = 18 * 18;
    // the raw patch of one 16-channel chunk is written by LDS-DMA loads (buffer_load_dwordx4 ... lds: 64 lanes x 16 bytes
    // land CONTIGUOUSLY, no padding possible), so bank spreading comes from the ORDER of the pixel slots instead: a patch
    // row holds 20 slots of 64 bytes and pixel x = 4a + c sits in slot 5c + a -- the four tiles of a 16-lane group read
    // x, x+4, x+8, x+12 = consecutive slots = four distinct 16-word bank groups, times four channel quads = all 64 banks.
    static constexpr int RAW_ROW = 20;                      // pixel slots per patch row (18 live)
    static constexpr int RAW_SLOTS = 18 * RAW_ROW;          // 360 live slots, written by 23 wave-wide loads of 16 slots
    static constexpr int RAW_LOADS = (RAW_SLOTS + 15) / 16; // 23
    static constexpr int RAW_FLOATS = RAW_LOADS * 16 * WINO4_KC;   // buffer padded to whole loads (dead lanes write zeros)
    static constexpr int RAW_ITERS = (RAW_LOADS + 3) / 4;   // loads per wave (6; wave 3 skips its last)
    static constexpr size_t LDS_BYTES = sizeof(float) * (2 * VBUF + 2 * RAW_FLOATS);
    static constexpr int HEAD_ROW = head_row(64);           // floats per pixel of the fused head's LDS tile
};

// ---- the raw patch: wave-wide load `load` (0 .. RAW_LOADS - 1) fills 16 slots, four lanes (ln & 3 = channel quad) per slot.
// Slot map: linear slot g -> patch pixel (py, px), its liveness, and the byte offset of the lane's channel quad in the image
// (chunk 0; 0xFFFFFFFF = reads zeros).  conv_wino4s.hip's fused first layer keeps a written-out copy of the map (see there).
// (Returned as a struct: as a plain `unsigned` result the same body makes both kernels 16 - 33 instructions longer.)
struct W4Slot {
    int g, py, px;      // linear slot, patch pixel
    bool inb;           // a live slot whose pixel lies inside the image
    unsigned voff;
};
static __device__ inline W4Slot w4_raw_slot(const ConvArgs a, const int by0, const int bx0, const int load, const int ln)
{
    W4Slot r;
    r.g = load * 16 + (ln >> 2);
    r.py = r.g / W4::RAW_ROW;
    const int sl = r.g - r.py * W4::RAW_ROW;
    r.px = 4 * (sl % 5) + sl / 5;
    const int gy = by0 - 1 + r.py, gx = bx0 - 1 + r.px;
    r.inb = r.g < W4::RAW_SLOTS && r.px < 18 && gy >= 0 && gy < a.H && gx >= 0 && gx < a.W;
    r.voff = r.inb ? (unsigned)(((gy * a.W + gx) * a.ldc + 4 * (ln & 3)) * 4) : 0xFFFFFFFFu;
    return r;
}
// one LDS-DMA load of a chunk's patch into the image at `raw`: global -> LDS directly, no registers, no ds_write; completion =
// vmcnt.  voff = the lane's W4Slot::voff of this load; c_ok = raw_chunk_ok: channels past Cin read zeros through the range
// check.  (The predicate is the caller's: computed in here, hipcc sinks it behind the branch of every load of a burst.)
static __device__ inline bool raw_chunk_ok(const int Cin, const int chunk, const int lane) { return chunk * WINO4_KC + 4 * (lane & 3) < Cin; }
static __device__ inline void raw_dma_one(const __amdgpu_buffer_rsrc_t in_rsrc, float *const raw, const int chunk, const int load,
                                          const unsigned voff, const bool c_ok)
{
    typedef __attribute__((address_space(3))) void *lds_ptr;
    if (load < W4::RAW_LOADS)
        __builtin_amdgcn_raw_ptr_buffer_load_lds(in_rsrc, (lds_ptr)(raw + load * 16 * WINO4_KC), 16, c_ok ? voff : 0xFFFFFFFFu,
                                                 chunk * WINO4_KC * 4, 0, 0);
}

// ---- forward transform V = B^T d B of one 16-channel chunk; lane = (tile, channel quad), wave role = row group of B^T:
//   role 0: xi 1, 2 = (d4 - 4 d2) +- (d3 - 4 d1)        role 1: xi 3, 4 = (d4 - d2) +- (2 d3 - 2 d1)
//   role 2: xi 0    = 4 d0 - 5 d2 + d4                  role 3: xi 5    = 4 d1 - 5 d3 + d5
struct W4Role {
    bool two;                   // a two-row role
    float c_alpha, c_beta;      // the two-row roles' wave-uniform coefficients
    int rd_off;                 // floats from the raw image to the lane's first patch pixel (row0, column 4 tx, quad)
    int rstride;                // floats between the rows the role reads (every row, or every second)
    int wr_off;                 // floats from V to the lane's row a, nu = 0 (+ nu * VPOS; row b = + 6 * VPOS)
};
static __device__ inline W4Role w4_role(const int wrole, const int lane)
{
    W4Role r;
    r.two = wrole < 2;
    const int t_tile = lane >> 2, t_quad = lane & 3;
    const int row0 = r.two ? 1 : wrole - 2, rstep = r.two ? 1 : 2;
    r.rd_off = (((4 * (t_tile >> 2) + row0) * W4::RAW_ROW + (t_tile & 3)) * 4 + t_quad) * 4;
    r.rstride = rstep * W4::RAW_ROW * WINO4_KC;
    const int xi_a = r.two ? (wrole == 0 ? 1 : 3) : (wrole == 2 ? 0 : 5);
    r.c_alpha = wrole == 0 ? -4.f : -1.f;
    r.c_beta = wrole == 0 ? 1.f : 2.f;
    r.wr_off = xi_a * 6 * W4::VPOS + t_tile * W4::VROW + 4 * (t_quad ^ v_swz(t_tile));
    return r;
}
// patch column k of the lane's rows: pixel 4 tx + k -> slot 5 (k & 3) + tx + (k >> 2).  (The one-row roles read a fourth row
// they never use, patch rows 6, 7: cheaper than a branch per column.)
static __device__ inline void w4_col_load(const float *const p_rd, const int rstride, const int k, f32x4 (&d)[4])
{
    const float *src = p_rd + ((k & 3) * 5 + (k >> 2)) * WINO4_KC;
    d[0] = *reinterpret_cast<const f32x4 *>(src);
    d[1] = *reinterpret_cast<const f32x4 *>(src + rstride);
    d[2] = *reinterpret_cast<const f32x4 *>(src + 2 * rstride);
    d[3] = *reinterpret_cast<const f32x4 *>(src + 3 * rstride);
}
// column step: rows a and b of B^T d for one patch column.  Roles 0 and 1 run ONE instruction sequence with wave-uniform
// coefficients (alpha, beta) = (-4, 1) and (-1, 2): ta = d3 + alpha d1, tb = d2 + alpha d0, rows ta +- beta tb.  The same values
// bit for bit as the literal forms (a product by 1 or -1 is exact), without role branches in front of every column (same-card
// A/B of a build where every wave took one role: -0.28 ms of the 10.9 ms the two-block kernel takes per step).
// The role's constants arrive as scalars: taken through a W4Role reference, the staged kernel spills (68-88 bytes of scratch).
static __device__ inline void w4_col(const bool two, const float c_alpha, const float c_beta, const f32x4 (&d)[4], f32x4 &ra, f32x4 &rb)
{
    if (two) {
        const f32x4 ta = d[3] + c_alpha * d[1];
        const f32x4 tb = d[2] + c_alpha * d[0];
        ra = ta + c_beta * tb;
        rb = ta - c_beta * tb;
    } else {
        ra = 4.f * d[0] - 5.f * d[1] + d[2];
        rb = ra;
    }
}
// row pass over one row c of B^T d: the four shared sub-expressions, then output nu (a constant at every call)
static __device__ inline void w4_row_prep(const f32x4 (&c)[6], f32x4 (&e)[4])
{
    e[0] = c[4] - 4.f * c[2]; e[1] = c[3] - 4.f * c[1]; e[2] = pk_sub(c[4], c[2]); e[3] = pk_sub(c[3], c[1]);
}
static __device__ inline f32x4 w4_row_out(const f32x4 (&c)[6], const f32x4 (&e)[4], const int nu)
{
    return nu == 0 ? 4.f * c[0] - 5.f * c[2] + c[4]
         : nu == 1 ? e[0] + e[1]
         : nu == 2 ? pk_sub(e[0], e[1])
         : nu == 3 ? e[2] + 2.f * e[3]
         : nu == 4 ? e[2] - 2.f * e[3]
                   : 4.f * c[1] - 5.f * c[3] + c[5];
}
// the whole row pass back to back: six 16-byte stores at dst + nu * VPOS.  (Written as six calls: as a loop over nu the staged
// kernel spills.)
static __device__ inline void w4_row_pass(const f32x4 (&c)[6], float *const dst)
{
    f32x4 e[4];
    w4_row_prep(c, e);
    *reinterpret_cast<f32x4 *>(dst + 0 * W4::VPOS) = w4_row_out(c, e, 0);
    *reinterpret_cast<f32x4 *>(dst + 1 * W4::VPOS) = w4_row_out(c, e, 1);
    *reinterpret_cast<f32x4 *>(dst + 2 * W4::VPOS) = w4_row_out(c, e, 2);
    *reinterpret_cast<f32x4 *>(dst + 3 * W4::VPOS) = w4_row_out(c, e, 3);
    *reinterpret_cast<f32x4 *>(dst + 4 * W4::VPOS) = w4_row_out(c, e, 4);
    *reinterpret_cast<f32x4 *>(dst + 5 * W4::VPOS) = w4_row_out(c, e, 5);
}

// ---- U fragments: 16-byte buffer loads from the layer's packed U [Cin/16][36][CoutPad][16] with scalar offsets
static __device__ inline __amdgpu_buffer_rsrc_t w4_u_rsrc(const ConvArgs a)
{
    const int chunks = (a.Cin + WINO4_KC - 1) / WINO4_KC;
    return __builtin_amdgcn_make_buffer_rsrc(const_cast<float *>(a.wpk4), 0, (int)(chunks * 36 * ((unsigned)a.CoutPad * WINO4_KC * 4)),
                                             0x00020000);
}
static __device__ inline f32x4 w4_u_load(const __amdgpu_buffer_rsrc_t u_rsrc, const unsigned voff, const unsigned pos_bytes,
                                         const int chunk, const int p)
{
    return __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(u_rsrc, voff, (chunk * 36 + p) * pos_bytes, 0));
}

// position (xi, nu) = (1, 1) starts at the shift: A^T e_1 e_1^T A is the all-ones tile, so the bias add is free
static __device__ inline float w4_acc_init(const ConvArgs a, const int p, const int ncol)
{
    return (p == 7 && ncol < a.Cout) ? a.bias[ncol] : 0.f;
}

// ---- epilogue: Y = A^T M A in-lane on all four tiles of a lane at once (the accumulator's four registers = tile columns
// r = 0..3 of tile row kq, lane = channel), ReLU, 4x4 stores (+ the 2x2 pooled maxima).  The shift was the initial value of
// position (1,1).  Stores are buffer stores on a per-image descriptor: one per-lane byte offset for the whole tile row, the
// pixel displacement in the scalar offset; pixels past the image edge and masked channels get voffset 0xFFFFFFFF, which the
// range check drops.
struct W4Out {                                      // (the two descriptors travel beside it: hipcc keeps a struct that holds one in scratch)
    int ld, co_off;                                 // floats per output pixel, first output channel
    int by0, bx0;                                   // the workgroup's 16x16 block
    float relu_lo;
    bool do_pool;
};
// One 16-channel block: position p's accumulator is acc[p * STRIDE]; lane = output channel ncol.  HEAD: the post-ReLU values
// go to column head_col of the head's LDS tile (fused_head_tile, kernel_common.h) instead of memory.  AUX = the stores' aux operand.
template <bool INTERIOR, bool HEAD, int AUX, int STRIDE>
static __device__ inline void w4_epilogue_block(const ConvArgs a, const W4Out &o, const __amdgpu_buffer_rsrc_t out_rsrc,
                                                const __amdgpu_buffer_rsrc_t pool_rsrc, const f32x4 *const acc, const int ncol,
                                                const int head_col, const int kq, float *const head_tile)
{
    const int Wp = a.W >> 1;
    const unsigned pix_bytes = (unsigned)o.ld * 4, row_bytes = (unsigned)a.W * pix_bytes;
    const unsigned ppix_bytes = (unsigned)a.pool_ld * 4, prow_bytes = (unsigned)Wp * ppix_bytes;
    const int oy = o.by0 + 4 * kq;
    const bool n_ok = ncol < a.Cout;
    const unsigned vbase = n_ok ? (unsigned)((oy * a.W + o.bx0) * o.ld + o.co_off + ncol) * 4 : 0xFFFFFFFFu;
    const unsigned pbase = n_ok ? (unsigned)(((oy >> 1) * Wp + (o.bx0 >> 1)) * a.pool_ld + ncol) * 4 : 0xFFFFFFFFu;
    unsigned vcol[4][4], pcol[4][2];          // edge workgroups: per-column offsets (dead columns -> dropped stores)
    if constexpr (!INTERIOR) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
#pragma unroll
            for (int k = 0; k < 4; ++k) vcol[r][k] = o.bx0 + 4 * r + k < a.W ? vbase : 0xFFFFFFFFu;
            pcol[r][0] = o.bx0 + 4 * r + 1 < a.W ? pbase : 0xFFFFFFFFu;
            pcol[r][1] = o.bx0 + 4 * r + 3 < a.W ? pbase : 0xFFFFFFFFu;
        }
    }
    // two tile columns (r = 2 h2, 2 h2 + 1) at a time: the same packed instructions as four at once, half the live
    // temporaries (the epilogue runs with every accumulator still resident)
#pragma unroll
    for (int h2 = 0; h2 < 2; ++h2) {
        auto half = [&](const f32x4 &v) { return h2 ? v.hi : v.lo; };
        f32x2 t[4][6];
#pragma unroll
        for (int nu = 0; nu < 6; ++nu) {
            const f32x2 m0 = half(acc[nu * STRIDE]), m1 = half(acc[(6 + nu) * STRIDE]), m2 = half(acc[(12 + nu) * STRIDE]),
                        m3 = half(acc[(18 + nu) * STRIDE]), m4 = half(acc[(24 + nu) * STRIDE]), m5 = half(acc[(30 + nu) * STRIDE]);
            const f32x2 s12 = m1 + m2, d12 = pk_sub2(m1, m2), s34 = m3 + m4, d34 = pk_sub2(m3, m4);
            t[0][nu] = m0 + s12 + s34;
            t[1][nu] = d12 + 2.f * d34;
            t[2][nu] = s12 + 4.f * s34;
            t[3][nu] = d12 + 8.f * d34 + m5;
        }
        f32x2 carry0, carry1;                 // horizontal maxima of the even row, for the 2x2 pooling
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const f32x2 s12 = t[i][1] + t[i][2], d12 = pk_sub2(t[i][1], t[i][2]), s34 = t[i][3] + t[i][4], d34 = pk_sub2(t[i][3], t[i][4]);
            f32x2 y[4];
            y[0] = t[i][0] + s12 + s34;
            y[1] = d12 + 2.f * d34;
            y[2] = s12 + 4.f * s34;
            y[3] = d12 + 8.f * d34 + t[i][5];
            const bool row_ok = INTERIOR || oy + i < a.H;      // per-lane (kq) row predicate of an edge workgroup
#pragma unroll
            for (int k = 0; k < 4; ++k)
#pragma unroll
                for (int rr = 0; rr < 2; ++rr) {
                    const int r = 2 * h2 + rr;
                    const float v = fmaxf(y[k][rr], o.relu_lo);
                    y[k][rr] = v;
                    if constexpr (HEAD) {     // pixel (4 kq + i, 4 r + k) of the 16x16 block, channel head_col -> LDS
                        head_tile[((4 * kq + i) * 16 + 4 * r + k) * W4::HEAD_ROW + head_col] = v;
                        continue;
                    }
                    unsigned voff = vbase;
                    if constexpr (!INTERIOR) voff = row_ok ? vcol[r][k] : 0xFFFFFFFFu;
                    __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(unsigned, v), out_rsrc, voff,
                                                          i * row_bytes + (4 * r + k) * pix_bytes, AUX);
                }
            if (!HEAD && o.do_pool) {
                f32x2 hm0, hm1;               // horizontal maxima of this row: pooled columns 2r and 2r + 1
#pragma unroll
                for (int rr = 0; rr < 2; ++rr) { hm0[rr] = fmaxf(y[0][rr], y[1][rr]); hm1[rr] = fmaxf(y[2][rr], y[3][rr]); }
                if ((i & 1) == 0) { carry0 = hm0; carry1 = hm1; }
                else {
#pragma unroll
                    for (int rr = 0; rr < 2; ++rr) {
                        const int r = 2 * h2 + rr;
                        const float p0 = fmaxf(hm0[rr], carry0[rr]), p1 = fmaxf(hm1[rr], carry1[rr]);
                        unsigned v0 = pbase, v1 = pbase;
                        if constexpr (!INTERIOR) { v0 = row_ok ? pcol[r][0] : 0xFFFFFFFFu; v1 = row_ok ? pcol[r][1] : 0xFFFFFFFFu; }
                        __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(unsigned, p0), pool_rsrc, v0,
                                                              (i >> 1) * prow_bytes + (2 * r) * ppix_bytes, AUX);
                        __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(unsigned, p1), pool_rsrc, v1,
                                                              (i >> 1) * prow_bytes + (2 * r + 1) * ppix_bytes, AUX);
                    }
                }
            }
        }
    }
}
// A wave's NB blocks (block blk: accumulators acc[p * NB + blk], channel ncol0 + 16 blk).  An interior workgroup (always, with
// HEAD: its tile is written whole) stores without per-pixel predicates; the choice is workgroup-uniform.
template <bool HEAD, int AUX, int NB>
static __device__ inline void w4_epilogue(const ConvArgs a, const W4Out &o, const __amdgpu_buffer_rsrc_t out_rsrc,
                                          const __amdgpu_buffer_rsrc_t pool_rsrc, const f32x4 *const acc, const int ncol0,
                                          const int head_col, const int kq, float *const head_tile)
{
    auto blocks = [&](auto interior_tag) {
#pragma unroll
        for (int blk = 0; blk < NB; ++blk)
            w4_epilogue_block<decltype(interior_tag)::value, HEAD, AUX, NB>(a, o, out_rsrc, pool_rsrc, acc + blk, ncol0 + 16 * blk, head_col, kq, head_tile);
    };
    if (HEAD || (o.by0 + 16 <= a.H && o.bx0 + 16 <= a.W)) blocks(std::true_type{});
    else blocks(std::false_type{});
}

}  // namespace miunet
