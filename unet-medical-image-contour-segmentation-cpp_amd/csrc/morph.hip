// morph.hip -- the closing and opening of postprocess_mask with a per-target radius and a box or Euclidean-disc element
// (include/mi_unet.h: mi_unet_set_morph).  Byte work, integer-exact.  gfx950 only.
#include "../../include/mi_unet.h"
#include "kernel_common.h"

namespace miunet {

namespace mp {

constexpr int MT = 64;                                  // a workgroup owns MT x MT output pixels of one plane
constexpr int MAXR = POSTPROCESS_MORPH_MAX_R;
constexpr int S_ROWS = MT + 2 * MAXR;                   // staged rows: the block and its halo
constexpr int S_PITCH = 128;                            // >= MT + 2 * MAXR = 126 staged columns
constexpr int G_PITCH = 192;                            // 48 banks: the four rows a wave reads in pass 2 fall on disjoint banks
static_assert(MT + 2 * MAXR <= S_PITCH && 4 * (MT / 4 - 1) + 4 * ((2 * MAXR + 4 + 3) / 4) <= G_PITCH, "LDS rows too short");

// One erosion (DILATE = false) or dilation of every plane by its target's element.  A STOPPER is a background pixel for an erosion
// and a foreground pixel for a dilation; positions outside the image are never stoppers, which is both border rules at once (an
// erosion is constrained, and a dilation seeded, only by pixels inside the image).
//   stage  : s_stop[yy][xx] = pixel (y0 - r + yy, x0 - r + xx) is a stopper, for the block and a halo of r
//   pass 1 : g(x, y) = distance to the nearest stopper of column x within r rows, r + 1 when there is none: a running distance down
//            and up the column, so O(1) per pixel; a column is cut into four segments of 16 rows (one lane each, r rows of run-up)
//   pass 2 : the pixel is hit when some |dx| <= r has g(x + dx, y) <= r (box) or g(x + dx, y)^2 + dx^2 <= r^2 (disc); columns outside
//            the image hold r + 1 and never hit.  A lane owns four neighbouring pixels and reads their common window of 2 r + 4
//            distances once, as dwords
//   write  : 255 where an erosion was not hit / a dilation was; through LDS, so that the global stores are whole rows
// Shape and radius are those of the block's plane (plane p is target p % K): uniform per workgroup, picked from the table with
// selects.  A plane with r = 0 is copied.  No dynamically indexed private array: nothing lives in scratch memory.
template <bool DILATE>
__global__ __launch_bounds__(256) void k_morph_step(const uint8_t *__restrict__ src, uint8_t *__restrict__ dst, int H, int W, int tiles_x,
                                                    int tiles_y, TargetTable t, bool closing)
{
    __shared__ __attribute__((aligned(16))) uint8_t s_stop[S_ROWS * S_PITCH];      // later: the block's output bytes [MT][MT]
    __shared__ __attribute__((aligned(16))) uint8_t s_g[MT * G_PITCH];
    const int per = tiles_x * tiles_y;
    const int p = blockIdx.x / per, tt = blockIdx.x - p * per, ty = tt / tiles_x, tx = tt - ty * tiles_x;
    const int k = p % t.K;
    int r = closing ? t.close_r[0] : t.open_r[0], shape = t.shape[0];
#pragma unroll
    for (int j = 1; j < POSTPROCESS_MAX_TARGETS; ++j)
        if (k == j) { r = closing ? t.close_r[j] : t.open_r[j]; shape = t.shape[j]; }
    const int x0 = tx * MT, y0 = ty * MT;
    const size_t base = (size_t)p * H * W;
    const uint8_t *const sp = src + base;
    uint8_t *const dp = dst + base;
    const int tid = threadIdx.x;
    if (r == 0) {                                               // (workgroup-uniform)
        for (int i = tid; i < MT * MT; i += 256) {
            const int y = y0 + (i >> 6), x = x0 + (i & 63);
            if (y < H && x < W) dp[(size_t)y * W + x] = sp[(size_t)y * W + x];
        }
        return;
    }
    const int sw = MT + 2 * r;                                  // staged columns = staged rows
    {
        const int xx = tid & 127, gx = x0 - r + xx;
        const bool col_in = xx < sw && gx >= 0 && gx < W;
        for (int yy = tid >> 7; yy < sw; yy += 2) {
            const int gy = y0 - r + yy;
            uint8_t v = 0;
            if (col_in && gy >= 0 && gy < H) {
                const bool f = sp[(size_t)gy * W + gx] != 0;
                v = (DILATE ? f : !f) ? 1 : 0;
            }
            if (xx < sw) s_stop[yy * S_PITCH + xx] = v;
        }
    }
    __syncthreads();
    // pass 1: output row j of the block is staged row j + r
    for (int round = 0; round < 2; ++round) {
        const int col = tid & 127, j0 = 16 * ((tid >> 7) + 2 * round);
        if (col < sw) {
            int d = r + 1;
            for (int yy = j0; yy < j0 + 16 + r; ++yy) {        // down: starts r rows above the segment
                d = s_stop[yy * S_PITCH + col] ? 0 : min(d + 1, r + 1);
                if (yy >= j0 + r) s_g[(yy - r) * G_PITCH + col] = (uint8_t)d;
            }
            d = r + 1;
            for (int yy = j0 + 15 + 2 * r; yy >= j0 + r; --yy) {   // up: starts r rows below it
                d = s_stop[yy * S_PITCH + col] ? 0 : min(d + 1, r + 1);
                if (yy <= j0 + 15 + r) {
                    const int at = (yy - r) * G_PITCH + col;
                    s_g[at] = (uint8_t)min((int)s_g[at], d);
                }
            }
        }
    }
    __syncthreads();                                            // s_stop is free from here on
    // pass 2: output pixel 4 * xg + o of row y looks at staged columns 4 * xg + o + r + dx, dx = -r .. r: window byte jj = o + r + dx
    const int r2 = r * r;
    const int disc = shape == MI_UNET_MORPH_DISC ? -1 : 0;
    const int ndw = (2 * r + 4 + 3) >> 2;
    unsigned *const s_out = reinterpret_cast<unsigned *>(s_stop);
    for (int round = 0; round < 4; ++round) {
        const int task = tid + 256 * round, y = task >> 4, xg = task & 15;
        const unsigned *const win = reinterpret_cast<const unsigned *>(s_g + y * G_PITCH + 4 * xg);
        bool hit0 = false, hit1 = false, hit2 = false, hit3 = false;
        for (int q = 0; q < ndw; ++q) {
            const unsigned wd = win[q];
#pragma unroll
            for (int b = 0; b < 4; ++b) {
                const int gv = (int)((wd >> (8 * b)) & 0xFFu), jj = 4 * q + b, gg = gv * gv;
                const int d0 = jj - r, d1 = d0 - 1, d2 = d0 - 2, d3 = d0 - 3;       // dx of the four pixels
                hit0 |= (unsigned)(d0 + r) <= (unsigned)(2 * r) && gg + ((d0 * d0) & disc) <= r2;
                hit1 |= (unsigned)(d1 + r) <= (unsigned)(2 * r) && gg + ((d1 * d1) & disc) <= r2;
                hit2 |= (unsigned)(d2 + r) <= (unsigned)(2 * r) && gg + ((d2 * d2) & disc) <= r2;
                hit3 |= (unsigned)(d3 + r) <= (unsigned)(2 * r) && gg + ((d3 * d3) & disc) <= r2;
            }
        }
        const unsigned on = (hit0 ? 0xFFu : 0u) | (hit1 ? 0xFF00u : 0u) | (hit2 ? 0xFF0000u : 0u) | (hit3 ? 0xFF000000u : 0u);
        s_out[y * (MT / 4) + xg] = DILATE ? on : ~on;
    }
    __syncthreads();
    for (int i = tid; i < MT * MT; i += 256) {
        const int y = y0 + (i >> 6), x = x0 + (i & 63);
        if (y < H && x < W) dp[(size_t)y * W + x] = s_stop[i];
    }
}

}  // namespace mp

bool morph_is_default(const TargetTable &t)
{
    for (int k = 0; k < t.K; ++k)
        if (t.shape[k] != MI_UNET_MORPH_RECT || t.open_r[k] != 1 || t.close_r[k] != 0) return false;
    return true;
}

hipError_t launch_morph_chain(uint8_t *a, uint8_t *b, int planes, int H, int W, const TargetTable &t, uint8_t **result, hipStream_t s)
{
    if (!a || !b || !result || planes <= 0 || H <= 0 || W <= 0 || t.K < 1 || t.K > POSTPROCESS_MAX_TARGETS || planes % t.K)
        return hipErrorInvalidValue;
    if ((long long)planes * H * W > 0x7FFFFFFFLL) return hipErrorInvalidValue;
    int max_open = 0, max_close = 0;
    for (int k = 0; k < t.K; ++k) {
        if (t.shape[k] != MI_UNET_MORPH_RECT && t.shape[k] != MI_UNET_MORPH_DISC) return hipErrorInvalidValue;
        if (t.open_r[k] < 0 || t.open_r[k] > POSTPROCESS_MORPH_MAX_R || t.close_r[k] < 0 || t.close_r[k] > POSTPROCESS_MORPH_MAX_R)
            return hipErrorInvalidValue;
        max_open = t.open_r[k] > max_open ? t.open_r[k] : max_open;
        max_close = t.close_r[k] > max_close ? t.close_r[k] : max_close;
    }
    const int tiles_x = (W + mp::MT - 1) / mp::MT, tiles_y = (H + mp::MT - 1) / mp::MT;
    const dim3 g((unsigned)((long long)planes * tiles_x * tiles_y)), blk(256);      // <= planes * H * W < 2^31
    uint8_t *cur = a, *other = b;
    auto step = [&](bool dilate, bool closing) {
        if (dilate) hipLaunchKernelGGL(mp::k_morph_step<true>, g, blk, 0, s, cur, other, H, W, tiles_x, tiles_y, t, closing);
        else hipLaunchKernelGGL(mp::k_morph_step<false>, g, blk, 0, s, cur, other, H, W, tiles_x, tiles_y, t, closing);
        uint8_t *const x = cur; cur = other; other = x;
    };
    if (max_close > 0) { step(true, true); step(false, true); }         // close: dilate, then erode
    if (max_open > 0) { step(false, false); step(true, false); }        // open: erode, then dilate
    *result = cur;
    return hipGetLastError();
}

}  // namespace miunet
