// tiles.hip -- the device side of tiled inference (mi_unet_infer_tiled_*): cut a device-resident image into the
// overlapping tiles of tile_grid.h, put the per-tile results back together, and the full-size form of the RAW16 normalisation.
// gfx950 only.
//
// All three kernels move a few bytes per pixel and compute next to nothing, so what matters is the shape of the memory
// accesses.  Tile origins and ownership cuts are arbitrary pixel positions: one side of every copy is unaligned.  The aligned
// side decides the lane layout -- one lane per 16 aligned bytes, consecutive lanes on consecutive 16-byte groups, one
// global_store_dwordx4 each -- and the unaligned side is read as ALIGNED dwords (one more than the lane needs) that
// v_alignbyte_b32 shifts into place.  Neighbouring lanes re-read each other's edge dword from L1.  Shapes whose rows are not
// multiples of 16 bytes take the same kernels at 4 bytes or 1 byte per lane.
#include "kernel_common.h"
#include "tile_grid.h"

namespace miunet {
namespace {

template <int BYTES> struct Words;
template <> struct Words<16> { typedef uint4 v; };
template <> struct Words<8> { typedef uint2 v; };
template <> struct Words<4> { typedef uint32_t v; };

// NW dwords starting at byte address `a`, read as aligned dwords.  The dword behind the last full one is only touched when
// a is unaligned, and then it holds bytes the caller asked for: the read stays inside a buffer whose length is a multiple of 4.
template <int NW>
__device__ __forceinline__ void load_unaligned(const uint8_t *a, uint32_t (&out)[NW])
{
    const uintptr_t addr = reinterpret_cast<uintptr_t>(a);
    const unsigned shift = (unsigned)(addr & 3);
    const uint32_t *p = reinterpret_cast<const uint32_t *>(addr & ~(uintptr_t)3);
    uint32_t w[NW + 1];
#pragma unroll
    for (int k = 0; k < NW; ++k) w[k] = p[k];
    w[NW] = shift ? p[NW] : 0u;
#pragma unroll
    for (int k = 0; k < NW; ++k) out[k] = __builtin_amdgcn_alignbyte(w[k + 1], w[k], shift);
}

template <int NW>
__device__ __forceinline__ void store_words(uint8_t *a, const uint32_t (&v)[NW])
{
    typename Words<NW * 4>::v o;
    if constexpr (NW == 4) { o.x = v[0]; o.y = v[1]; o.z = v[2]; o.w = v[3]; }
    else if constexpr (NW == 2) { o.x = v[0]; o.y = v[1]; }
    else o = v[0];
    *reinterpret_cast<typename Words<NW * 4>::v *>(a) = o;
}

// image u8 [H][W][C] -> tiles t0 .. t0 + nb - 1 as u8 [nb][th][tw][C].  A tile row is tw * C contiguous bytes on both sides and
// the tile batch is dense, so lane e owns bytes [e * VEC, (e + 1) * VEC) of the batch; rpt = VEC-byte groups per tile row.
template <int VEC>
__global__ __launch_bounds__(256) void tile_gather_kernel(const uint8_t *__restrict__ img, uint8_t *__restrict__ tiles, TileGrid g, int C,
                                                          int t0, unsigned rpt, unsigned total)
{
    for (unsigned e = blockIdx.x * 256u + threadIdx.x; e < total; e += gridDim.x * 256u) {
        const unsigned r = e / rpt, c = e - r * rpt;
        const unsigned j = r / (unsigned)g.th, y = r - j * (unsigned)g.th;
        const int t = t0 + (int)j, ty = t / g.nx, tx = t - ty * g.nx;
        const int oy = tile_origin(g.H, g.th, g.sy, ty), ox = tile_origin(g.W, g.tw, g.sx, tx);
        const uint8_t *src = img + ((size_t)(oy + (int)y) * g.W + ox) * C + (size_t)c * VEC;
        if constexpr (VEC >= 4) {
            uint32_t v[VEC / 4];
            load_unaligned<VEC / 4>(src, v);
            store_words<VEC / 4>(tiles + (size_t)e * VEC, v);
        } else {
            tiles[e] = *src;
        }
    }
}

// The mirrored form (blending): views k0 .. k0 + nb - 1, nv views per tile (view v of tile t is k = t * nv + v), view
// v mirrored by the bits (flips >> 2v) & 3 (1: X, column j <- tw - 1 - j; 2: Y, row i <- th - 1 - i).  Same lane layout as above.
// An X-mirrored group of VEC bytes is the source group that ends where the output group starts, read the same way and byte-reversed;
// VEC > 1 with X mirrors needs C == 1 (the launcher's choice), a multi-byte pixel takes the byte-wise path.
template <int VEC>
__global__ __launch_bounds__(256) void tile_gather_views_kernel(const uint8_t *__restrict__ img, uint8_t *__restrict__ tiles, TileGrid g,
                                                                int C, int k0, int nv, unsigned flips, unsigned rpt, unsigned total)
{
    for (unsigned e = blockIdx.x * 256u + threadIdx.x; e < total; e += gridDim.x * 256u) {
        const unsigned r = e / rpt, c = e - r * rpt;
        const unsigned j = r / (unsigned)g.th, y = r - j * (unsigned)g.th;
        const int k = k0 + (int)j, t = k / nv, v = k - t * nv, ty = t / g.nx, tx = t - ty * g.nx;
        const unsigned f = (flips >> (2 * v)) & 3u;
        const int oy = tile_origin(g.H, g.th, g.sy, ty), ox = tile_origin(g.W, g.tw, g.sx, tx);
        const int sy = (f & 2u) ? g.th - 1 - (int)y : (int)y;
        const uint8_t *row = img + ((size_t)(oy + sy) * g.W + ox) * C;
        if constexpr (VEC >= 4) {
            uint32_t w[VEC / 4];
            if (!(f & 1u)) {
                load_unaligned<VEC / 4>(row + (size_t)c * VEC, w);
                store_words<VEC / 4>(tiles + (size_t)e * VEC, w);
            } else {
                load_unaligned<VEC / 4>(row + (size_t)g.tw - (size_t)(c + 1) * VEC, w);
                uint32_t o[VEC / 4];
#pragma unroll
                for (int q = 0; q < VEC / 4; ++q) o[q] = __builtin_bswap32(w[VEC / 4 - 1 - q]);
                store_words<VEC / 4>(tiles + (size_t)e * VEC, o);
            }
        } else {
            const unsigned x = c / (unsigned)C, ch = c - x * (unsigned)C;
            tiles[e] = row[(size_t)((f & 1u) ? (unsigned)g.tw - 1 - x : x) * C + ch];
        }
    }
}

// RAW16 -> u8 at the image's own size: resample_u8_kernel (image_stages.hip) at outW == w, outH == h, where dx = dy = 0 and the
// four-tap sum is the pixel itself.  The quantisation is that kernel's, operation for operation (fp64, one rounding each, no
// contraction); 8 samples per lane, one 16-byte load.
// WINDOW: an intensity window instead of the min/max stretch: the sample clamped to [lo, hi], as resample_u8_kernel<true>
template <bool WINDOW>
__device__ __forceinline__ uint8_t quantise_u16(unsigned v, double lo, double hi, double scale8)
{
    double x = (double)v;
    if constexpr (WINDOW) x = x < lo ? lo : x > hi ? hi : x;
    const double q = __dadd_rn(__dmul_rn(__dsub_rn(x, lo), scale8), 0.5);
    return (uint8_t)(int)q;
}

template <bool WINDOW>
__global__ __launch_bounds__(256) void normalise_u16_kernel(const uint16_t *__restrict__ raw, size_t n, const unsigned *__restrict__ mnmx,
                                                            int win_lo, int win_hi, uint8_t *__restrict__ dst, int dst_stride)
{
#pragma clang fp contract(off)
    double lo, hi = 0.0, scale8;
    if constexpr (WINDOW) {                                     // the pair of launch_window_select_u16, or (mnmx null) the arguments
        const int L = mnmx ? (int)mnmx[0] : win_lo, h0 = mnmx ? (int)mnmx[1] : win_hi;
        const int Hh = h0 > L ? h0 : L + 1;                     // evaluated in int: nothing wraps
        lo = (double)L; hi = (double)Hh;
        scale8 = 255.0 / (double)(Hh - L);
    } else {
        const unsigned short mn = (unsigned short)mnmx[0];
        unsigned short mx = (unsigned short)mnmx[1];
        if (mn == mx) mx = (unsigned short)(mn + 1);            // evaluated in uint16_t, as resample_u8_kernel does
        lo = (double)mn;
        scale8 = 255.0 / (double)((int)mx - (int)mn);
    }
    const size_t n8 = n / 8;
    const uint4 *v = reinterpret_cast<const uint4 *>(raw);
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n8; i += (size_t)gridDim.x * 256) {
        const uint4 q = v[i];
        const unsigned ws[4] = { q.x, q.y, q.z, q.w };
        uint8_t o[8];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            o[2 * k] = quantise_u16<WINDOW>(ws[k] & 0xFFFFu, lo, hi, scale8);
            o[2 * k + 1] = quantise_u16<WINDOW>(ws[k] >> 16, lo, hi, scale8);
        }
        if (dst_stride == 1) {                                  // planar: one 8-byte store
            uint2 p;
            p.x = o[0] | (o[1] << 8) | (o[2] << 16) | ((unsigned)o[3] << 24);
            p.y = o[4] | (o[5] << 8) | (o[6] << 16) | ((unsigned)o[7] << 24);
            *reinterpret_cast<uint2 *>(dst + i * 8) = p;
        } else {                                                // plane c of an interleaved image
#pragma unroll
            for (int k = 0; k < 8; ++k) dst[(i * 8 + k) * dst_stride] = o[k];
        }
    }
    if (blockIdx.x == 0 && threadIdx.x < (n & 7)) {             // ragged tail
        const size_t i = n8 * 8 + threadIdx.x;
        dst[i * dst_stride] = quantise_u16<WINDOW>(raw[i], lo, hi, scale8);
    }
}

// per-tile planes [nb][planes][th][tw] of ES-byte elements -> the rectangle each tile owns in [planes][H][W].  The destination is
// the aligned side: lane (tile, plane, row, i) covers the i-th VEC-aligned byte group of the destination row that touches the
// tile's owned columns.  A group that lies inside the owned columns is one wide store; the (at most two) groups per row that
// straddle a cut are written element by element, only the elements this tile owns -- the neighbouring tile writes the others in
// the same launch, so no byte is written twice and none is read back.  gpr = groups per row, an upper bound (tw * ES / VEC + 1).
template <int VEC, int ES>
__global__ __launch_bounds__(256) void tile_stitch_kernel(const uint8_t *__restrict__ src, uint8_t *__restrict__ dst, TileGrid g, int planes,
                                                          int t0, unsigned gpr, unsigned total)
{
    for (unsigned e = blockIdx.x * 256u + threadIdx.x; e < total; e += gridDim.x * 256u) {
        const unsigned r = e / gpr, i = e - r * gpr;
        const unsigned r2 = r / (unsigned)g.th, y = r - r2 * (unsigned)g.th;
        const unsigned j = r2 / (unsigned)planes, p = r2 - j * (unsigned)planes;
        const int t = t0 + (int)j, ty = t / g.nx, tx = t - ty * g.nx;
        const int oy = tile_origin(g.H, g.th, g.sy, ty), ox = tile_origin(g.W, g.tw, g.sx, tx);
        const int Y = oy + (int)y;
        if (Y < tile_cut(g.H, g.th, g.sy, g.ny, ty) || Y >= tile_cut(g.H, g.th, g.sy, g.ny, ty + 1)) continue;
        // owned columns as byte offsets into the destination row
        const int b0 = tile_cut(g.W, g.tw, g.sx, g.nx, tx) * ES, b1 = tile_cut(g.W, g.tw, g.sx, g.nx, tx + 1) * ES;
        const int x0 = (b0 / VEC + (int)i) * VEC;
        if (x0 >= b1) continue;
        const uint8_t *srow = src + ((size_t)r2 * g.th + y) * g.tw * ES - (size_t)ox * ES;       // indexed by destination byte offset
        uint8_t *drow = dst + ((size_t)p * g.H + Y) * g.W * ES;
        if (VEC >= 4 && x0 >= b0 && x0 + VEC <= b1) {
            if constexpr (VEC >= 4) {
                uint32_t v[VEC / 4];
                load_unaligned<VEC / 4>(srow + x0, v);
                store_words<VEC / 4>(drow + x0, v);
            }
        } else {
#pragma unroll
            for (int b = 0; b < VEC; b += ES) {
                const int X = x0 + b;
                if (X < b0 || X >= b1) continue;
                if constexpr (ES == 4) *reinterpret_cast<uint32_t *>(drow + X) = *reinterpret_cast<const uint32_t *>(srow + X);
                else drow[X] = srow[X];
            }
        }
    }
}

unsigned grid_for(unsigned total) { return (total + 255u) / 256u; }     // one lane per group, as upsample.hip; the kernels grid-stride anyway

template <int ES>
hipError_t stitch_typed(const void *src, void *dst, const TileGrid &g, int planes, int t0, int nb, hipStream_t s)
{
    const uintptr_t ps = reinterpret_cast<uintptr_t>(src), pd = reinterpret_cast<uintptr_t>(dst);
    const size_t drow = (size_t)g.W * ES, srow = (size_t)g.tw * ES;
    if (ps % ES || pd % ES) return hipErrorInvalidValue;
    // the widest group both sides allow: destination rows and base multiples of it, tile rows whole dwords
    int vec = ES == 1 ? 1 : 4;
    if (srow % 4 == 0 && ps % 4 == 0) {
        if (drow % 16 == 0 && pd % 16 == 0) vec = 16;
        else if (drow % 4 == 0 && pd % 4 == 0) vec = 4;
    }
    const unsigned long long gpr = srow / vec + 1, total = gpr * g.th * planes * nb;
    if (total >= (1ull << 31)) return hipErrorInvalidValue;
    const uint8_t *sb = static_cast<const uint8_t *>(src);
    uint8_t *db = static_cast<uint8_t *>(dst);
#define MIUNET_STITCH(V) \
    hipLaunchKernelGGL((tile_stitch_kernel<V, ES>), dim3(grid_for((unsigned)total)), dim3(256), 0, s, sb, db, g, planes, t0, (unsigned)gpr, (unsigned)total)
    if (vec == 16) MIUNET_STITCH(16);
    else if (vec == 4) MIUNET_STITCH(4);
    else if constexpr (ES == 1) MIUNET_STITCH(1);
#undef MIUNET_STITCH
    return hipGetLastError();
}

bool batch_ok(const TileGrid &g, int t0, int nb) { return t0 >= 0 && nb >= 0 && (long long)t0 + nb <= (long long)g.ny * g.nx; }

}  // namespace

hipError_t launch_tile_gather(const uint8_t *img, size_t img_bytes, int H, int W, int C, int th, int tw, int halo, int t0, int nb,
                              uint8_t *tiles, hipStream_t s)
{
    TileGrid g;
    if (!img || !tiles || C < 1 || C > 4 || !tile_grid(H, W, th, tw, halo, g) || !batch_ok(g, t0, nb)) return hipErrorInvalidValue;
    const size_t need = (size_t)H * W * C, row = (size_t)tw * C;
    if (img_bytes < need) return hipErrorInvalidValue;
    if (nb == 0) return hipSuccess;
    const uintptr_t pi = reinterpret_cast<uintptr_t>(img), pt = reinterpret_cast<uintptr_t>(tiles);
    // aligned-dword reads of the image need its base on a dword and its allocation to end on one
    const bool dwords = pi % 4 == 0 && img_bytes >= (need + 3) / 4 * 4 && row % 4 == 0;
    const int vec = !dwords ? 1 : (row % 16 == 0 && pt % 16 == 0) ? 16 : (row % 8 == 0 && pt % 8 == 0) ? 8 : pt % 4 == 0 ? 4 : 1;
    const unsigned long long rpt = row / vec, total = rpt * th * nb;
    if (total >= (1ull << 31)) return hipErrorInvalidValue;
#define MIUNET_GATHER(V) \
    hipLaunchKernelGGL(tile_gather_kernel<V>, dim3(grid_for((unsigned)total)), dim3(256), 0, s, img, tiles, g, C, t0, (unsigned)rpt, (unsigned)total)
    if (vec == 16) MIUNET_GATHER(16);
    else if (vec == 8) MIUNET_GATHER(8);
    else if (vec == 4) MIUNET_GATHER(4);
    else MIUNET_GATHER(1);
#undef MIUNET_GATHER
    return hipGetLastError();
}

hipError_t launch_tile_gather_views(const uint8_t *img, size_t img_bytes, int H, int W, int C, int th, int tw, int halo, int mirror,
                                    int k0, int nb, uint8_t *tiles, hipStream_t s)
{
    TileGrid g;
    if (!img || !tiles || C < 1 || C > 4 || mirror < 0 || mirror > 3 || !tile_grid(H, W, th, tw, halo, g)) return hipErrorInvalidValue;
    const int nv = tile_view_count(mirror);
    if (k0 < 0 || nb < 0 || (long long)k0 + nb > (long long)g.ny * g.nx * nv) return hipErrorInvalidValue;
    const size_t need = (size_t)H * W * C, row = (size_t)tw * C;
    if (img_bytes < need) return hipErrorInvalidValue;
    if (nb == 0) return hipSuccess;
    unsigned flips = 0;
    for (int v = 0; v < nv; ++v) flips |= (unsigned)tile_view_flip(mirror, v) << (2 * v);
    const uintptr_t pi = reinterpret_cast<uintptr_t>(img), pt = reinterpret_cast<uintptr_t>(tiles);
    const bool dwords = pi % 4 == 0 && img_bytes >= (need + 3) / 4 * 4 && row % 4 == 0 && (C == 1 || !(mirror & 1));
    const int vec = !dwords ? 1 : (row % 16 == 0 && pt % 16 == 0) ? 16 : (row % 8 == 0 && pt % 8 == 0) ? 8 : pt % 4 == 0 ? 4 : 1;
    const unsigned long long rpt = row / vec, total = rpt * th * nb;
    if (total >= (1ull << 31)) return hipErrorInvalidValue;
#define MIUNET_GATHER_VIEWS(V) \
    hipLaunchKernelGGL(tile_gather_views_kernel<V>, dim3(grid_for((unsigned)total)), dim3(256), 0, s, img, tiles, g, C, k0, nv, flips, (unsigned)rpt, (unsigned)total)
    if (vec == 16) MIUNET_GATHER_VIEWS(16);
    else if (vec == 8) MIUNET_GATHER_VIEWS(8);
    else if (vec == 4) MIUNET_GATHER_VIEWS(4);
    else MIUNET_GATHER_VIEWS(1);
#undef MIUNET_GATHER_VIEWS
    return hipGetLastError();
}

template <bool WINDOW>
static hipError_t normalise_u16(const uint16_t *raw, int w, int h, const unsigned *mnmx, int lo, int hi, uint8_t *dst, int dst_stride,
                                hipStream_t s)
{
    if (!raw || !dst || w <= 0 || h <= 0 || dst_stride < 1) return hipErrorInvalidValue;
    if (reinterpret_cast<uintptr_t>(raw) & 15) return hipErrorInvalidValue;
    if (dst_stride == 1 && (reinterpret_cast<uintptr_t>(dst) & 7)) return hipErrorInvalidValue;
    const size_t n = (size_t)w * h;
    size_t blocks = (n / 8 + 255) / 256;
    if (blocks == 0) blocks = 1;
    if (blocks >= (1u << 31)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(normalise_u16_kernel<WINDOW>, dim3((unsigned)blocks), dim3(256), 0, s, raw, n, mnmx, lo, hi, dst, dst_stride);
    return hipGetLastError();
}

hipError_t launch_normalise_u16(const uint16_t *raw, int w, int h, const unsigned *mnmx, uint8_t *dst, int dst_stride, hipStream_t s)
{
    if (!mnmx) return hipErrorInvalidValue;
    return normalise_u16<false>(raw, w, h, mnmx, 0, 0, dst, dst_stride, s);
}

hipError_t launch_normalise_u16_window(const uint16_t *raw, int w, int h, const unsigned *mnmx, int lo, int hi, uint8_t *dst,
                                       int dst_stride, hipStream_t s)
{
    if (!mnmx && (lo < 0 || lo > hi || hi > 65535)) return hipErrorInvalidValue;
    return normalise_u16<true>(raw, w, h, mnmx, lo, hi, dst, dst_stride, s);
}

hipError_t launch_tile_stitch(const uint8_t *tile_labels, const float *tile_logits, int classes, int H, int W, int th, int tw, int halo,
                              int t0, int nb, uint8_t *labels, float *logits, hipStream_t s)
{
    TileGrid g;
    if (!tile_labels || !labels || !tile_grid(H, W, th, tw, halo, g) || !batch_ok(g, t0, nb)) return hipErrorInvalidValue;
    if ((tile_logits != nullptr) != (logits != nullptr) || (logits && classes < 1)) return hipErrorInvalidValue;
    if (nb == 0) return hipSuccess;
    hipError_t e = stitch_typed<1>(tile_labels, labels, g, 1, t0, nb, s);
    if (e == hipSuccess && logits) e = stitch_typed<4>(tile_logits, logits, g, classes, t0, nb, s);
    return e;
}

}  // namespace miunet
