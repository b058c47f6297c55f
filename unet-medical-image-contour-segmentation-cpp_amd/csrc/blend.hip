// blend.hip -- the device side of blended tiled inference (mi_unet_set_tile_blend): the per-view logits of each
// micro-batch are un-mirrored and added, weighted, into one full-size fp32 accumulator; after the last micro-batch every pixel is
// divided by its weight sum and labelled.  gfx950 only.
//
// Both kernels are destination-centric: a lane owns one image pixel and walks, per class, the views that cover it in increasing view
// index k = t * nv + v, so the order of every sum is fixed by the definition in include/mi_unet.h and not by the launch -- no atomics,
// one read-modify-write of the accumulator per covered pixel and micro-batch.  The weight sum is not stored: blend_finalize adds the
// same weights again in the same order over all views, which gives the same float as a stored plane would.
#include "kernel_common.h"
#include "tile_grid.h"

namespace miunet {
namespace {

struct Span { int lo, hi; };

// the tiles of one axis that contribute to position pos: every tile that covers it, or (owner) the one tile that owns it
__device__ __forceinline__ Span contributors(int L, int T, int S, int n, int pos, bool owner)
{
    Span sp{ tile_first_cover(T, S, pos), tile_last_cover(L, T, S, n, pos) };
    if (owner) {
        while (sp.lo < sp.hi && pos >= tile_cut(L, T, S, n, sp.lo + 1)) ++sp.lo;
        sp.hi = sp.lo;
    }
    return sp;
}

// views k0 .. k0 + nb - 1: src = their planar logits [nb][classes][th][tw], view v of a tile mirrored by (flips >> 2v) & 3 (1: X,
// 2: Y) -> acc [classes][H][W] += w * logit, w = wy[i] * wx[j] (owner: 1).  Lanes cover image rows row0 .. row0 + total / W - 1,
// the rows the micro-batch's tiles span.
__global__ __launch_bounds__(256) void tile_blend_kernel(const float *__restrict__ src, float *__restrict__ acc, const float *__restrict__ wy,
                                                         const float *__restrict__ wx, TileGrid g, int classes, int nv, unsigned flips,
                                                         int owner, int k0, int nb, int row0, unsigned total)
{
#pragma clang fp contract(off)
    const int k1 = k0 + nb, tA = k0 / nv, tB = (k1 - 1) / nv;
    const size_t plane = (size_t)g.H * g.W, tplane = (size_t)g.th * g.tw;
    for (unsigned e = blockIdx.x * 256u + threadIdx.x; e < total; e += gridDim.x * 256u) {
        const int Y = row0 + (int)(e / (unsigned)g.W), X = (int)(e % (unsigned)g.W);
        const Span sy = contributors(g.H, g.th, g.sy, g.ny, Y, owner), sx = contributors(g.W, g.tw, g.sx, g.nx, X, owner);
        // every tile in [tA, tB] has at least one view in [k0, k1): the pixel is touched iff one of its tiles lies there
        bool any = false;
        for (int ty = sy.lo; ty <= sy.hi; ++ty) any |= ty * g.nx + sx.lo <= tB && ty * g.nx + sx.hi >= tA;
        if (!any) continue;
        float *a_px = acc + (size_t)Y * g.W + X;
        for (int c = 0; c < classes; ++c) {
            float a = a_px[c * plane];
            for (int ty = sy.lo; ty <= sy.hi; ++ty) {
                const int i = Y - tile_origin(g.H, g.th, g.sy, ty);
                for (int tx = sx.lo; tx <= sx.hi; ++tx) {
                    const int t = ty * g.nx + tx;
                    if (t < tA || t > tB) continue;
                    const int j = X - tile_origin(g.W, g.tw, g.sx, tx);
                    const float w = owner ? 1.f : wy[i] * wx[j];
                    for (int v = 0; v < nv; ++v) {
                        const int k = t * nv + v;
                        if (k < k0 || k >= k1) continue;
                        const unsigned f = (flips >> (2 * v)) & 3u;
                        const int si = (f & 2u) ? g.th - 1 - i : i, sj = (f & 1u) ? g.tw - 1 - j : j;
                        a = a + w * src[((size_t)(k - k0) * classes + c) * tplane + (size_t)si * g.tw + sj];
                    }
                }
            }
            a_px[c * plane] = a;
        }
    }
}

// acc [classes][H][W] -> logit = acc / (the same weights summed over every view in k order), correctly rounded; labels [H][W] = the
// argmax of head_argmax_kernel (strict '>' from -FLT_MAX in class order); logits [classes][H][W] when not null (may be acc itself)
__global__ __launch_bounds__(256) void blend_finalize_kernel(const float *acc, const float *__restrict__ wy, const float *__restrict__ wx,
                                                             TileGrid g, int classes, int nv, int owner, uint8_t *__restrict__ labels,
                                                             float *logits, unsigned total)
{
#pragma clang fp contract(off)
    const size_t plane = (size_t)g.H * g.W;
    for (unsigned e = blockIdx.x * 256u + threadIdx.x; e < total; e += gridDim.x * 256u) {
        const int Y = (int)(e / (unsigned)g.W), X = (int)(e % (unsigned)g.W);
        const Span sy = contributors(g.H, g.th, g.sy, g.ny, Y, owner), sx = contributors(g.W, g.tw, g.sx, g.nx, X, owner);
        float ws = 0.f;
        for (int ty = sy.lo; ty <= sy.hi; ++ty) {
            const int i = Y - tile_origin(g.H, g.th, g.sy, ty);
            for (int tx = sx.lo; tx <= sx.hi; ++tx) {
                const float w = owner ? 1.f : wy[i] * wx[X - tile_origin(g.W, g.tw, g.sx, tx)];
                for (int v = 0; v < nv; ++v) ws = ws + w;
            }
        }
        float best = -3.402823466e+38f;
        int idx = 0;
        for (int c = 0; c < classes; ++c) {
            const float r = __fdiv_rn(acc[c * plane + e], ws);
            if (logits) logits[c * plane + e] = r;
            if (r > best) { best = r; idx = c; }
        }
        labels[e] = (uint8_t)idx;
    }
}

unsigned lanes_grid(unsigned total) { return (total + 255u) / 256u; }

}  // namespace

hipError_t launch_tile_blend(const float *tile_logits, int classes, int H, int W, int th, int tw, int halo, int mirror, bool owner,
                             const float *wy, const float *wx, int k0, int nb, float *acc, hipStream_t s)
{
    TileGrid g;
    if (!tile_logits || !acc || classes < 1 || mirror < 0 || mirror > 3 || (!owner && (!wy || !wx)) || !tile_grid(H, W, th, tw, halo, g))
        return hipErrorInvalidValue;
    const int nv = tile_view_count(mirror);
    if (k0 < 0 || nb < 0 || (long long)k0 + nb > (long long)g.ny * g.nx * nv) return hipErrorInvalidValue;
    if (nb == 0) return hipSuccess;
    unsigned flips = 0;
    for (int v = 0; v < nv; ++v) flips |= (unsigned)tile_view_flip(mirror, v) << (2 * v);
    const int tA = k0 / nv, tB = (k0 + nb - 1) / nv;
    const int row0 = tile_origin(H, th, g.sy, tA / g.nx), row1 = tile_origin(H, th, g.sy, tB / g.nx) + th;
    const unsigned long long total = (unsigned long long)(row1 - row0) * W;
    if (total >= (1ull << 31)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(tile_blend_kernel, dim3(lanes_grid((unsigned)total)), dim3(256), 0, s, tile_logits, acc, wy, wx, g, classes, nv, flips,
                       (int)owner, k0, nb, row0, (unsigned)total);
    return hipGetLastError();
}

hipError_t launch_blend_finalize(const float *acc, int classes, int H, int W, int th, int tw, int halo, int mirror, bool owner,
                                 const float *wy, const float *wx, uint8_t *labels, float *logits, hipStream_t s)
{
    TileGrid g;
    if (!acc || !labels || classes < 1 || mirror < 0 || mirror > 3 || (!owner && (!wy || !wx)) || !tile_grid(H, W, th, tw, halo, g))
        return hipErrorInvalidValue;
    const unsigned long long total = (unsigned long long)H * W;
    if (total >= (1ull << 31)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(blend_finalize_kernel, dim3(lanes_grid((unsigned)total)), dim3(256), 0, s, acc, wy, wx, g, classes,
                       tile_view_count(mirror), (int)owner, labels, logits, (unsigned)total);
    return hipGetLastError();
}

}  // namespace miunet
