// image_stages.hip -- the reference's CPU-side image stages on the device: RAW16 preprocessing (f1), postprocess_mask
// (f2), mask_to_image + extract_contours (f3).  Integer / byte / fp64 work, bit-exact against the oracle.  gfx950 only.
#include "cc_common.h"
#include "kernel_common.h"
#include "wave.h"

namespace miunet {

// --------------------------------------------------------------------------------------------------------------------
// RAW16 preprocessing on the device: HBM-bound integer scan + a 262144-pixel fp64 gather.
__global__ __launch_bounds__(256) void minmax_init_kernel(unsigned *mnmx)
{
    if (threadIdx.x == 0) { mnmx[0] = 65535u; mnmx[1] = 0u; }
}

__global__ __launch_bounds__(256) void minmax_u16_kernel(const uint16_t *__restrict__ raw, size_t n, unsigned *mnmx)
{
    __shared__ unsigned s_lo[4], s_hi[4];
    unsigned lo = 65535u, hi = 0u;
    const size_t n8 = n / 8;                                   // 16 bytes = 8 samples per lane
    const uint4 *v = reinterpret_cast<const uint4 *>(raw);
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n8; i += (size_t)gridDim.x * 256) {
        const uint4 q = v[i];
        const unsigned ws[4] = { q.x, q.y, q.z, q.w };
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const unsigned a = ws[k] & 0xFFFFu, b = ws[k] >> 16;
            lo = min(lo, min(a, b));
            hi = max(hi, max(a, b));
        }
    }
    if (blockIdx.x == 0 && threadIdx.x < (n & 7)) {            // ragged tail
        const unsigned a = raw[n8 * 8 + threadIdx.x];
        lo = min(lo, a); hi = max(hi, a);
    }
    lo = wave::wave_min(lo);
    hi = wave::wave_max(hi);
    if ((threadIdx.x & 63) == 0) { s_lo[threadIdx.x >> 6] = lo; s_hi[threadIdx.x >> 6] = hi; }
    __syncthreads();
    if (threadIdx.x == 0) {                                     // ONE atomic pair per workgroup: same-address atomics serialise
        atomicMin(&mnmx[0], min(min(s_lo[0], s_lo[1]), min(s_lo[2], s_lo[3])));
        atomicMax(&mnmx[1], max(max(s_hi[0], s_hi[1]), max(s_hi[2], s_hi[3])));
    }
}

hipError_t launch_minmax_u16(const uint16_t *raw, size_t n, unsigned *mnmx, hipStream_t s)
{
    if (n == 0 || (reinterpret_cast<uintptr_t>(raw) & 15)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(minmax_init_kernel, dim3(1), dim3(256), 0, s, mnmx);
    size_t blocks = (n / 8 + 255) / 256;
    if (blocks > 512) blocks = 512;
    if (blocks == 0) blocks = 1;
    hipLaunchKernelGGL(minmax_u16_kernel, dim3((unsigned)blocks), dim3(256), 0, s, raw, n, mnmx);
    return hipGetLastError();
}

// WINDOW = false: the reference's min/max stretch (mnmx = launch_minmax_u16's pair).  WINDOW = true: an intensity window (DESIGN.md
// 7.5) -- the pair from launch_window_select_u16's slot or, with mnmx null, the arguments win_lo / win_hi -- with the interpolant
// clamped to it; the degenerate-window bump is evaluated in int there, so nothing wraps.
template <bool WINDOW>
__global__ __launch_bounds__(256) void resample_u8_kernel(const uint16_t *__restrict__ raw, int w, int h,
                                                          const unsigned *__restrict__ mnmx, int win_lo, int win_hi,
                                                          uint8_t *__restrict__ dst, int outW, int outH, int dst_stride)
{
#pragma clang fp contract(off)
    const int x = blockIdx.x * 64 + (threadIdx.x & 63);
    const int y = blockIdx.y * 4 + (threadIdx.x >> 6);
    if (x >= outW || y >= outH) return;
    double lo8, hi8 = 0.0, scale8;
    if constexpr (WINDOW) {
        const int L = mnmx ? (int)mnmx[0] : win_lo, hi = mnmx ? (int)mnmx[1] : win_hi;
        const int Hh = hi > L ? hi : L + 1;
        lo8 = (double)L; hi8 = (double)Hh;
        scale8 = 255.0 / (double)(Hh - L);
    } else {
        const unsigned short mn = (unsigned short)mnmx[0];
        unsigned short mx = (unsigned short)mnmx[1];
        if (mn == mx) mx = (unsigned short)(mn + 1);            // evaluated in uint16_t: wraps to 0 at 65535 (src/preprocess.cpp:92)
        lo8 = (double)mn;
        scale8 = 255.0 / (double)((int)mx - (int)mn);
    }
    const double stepX = (double)w / (double)outW, stepY = (double)h / (double)outH;
    const double fx = __dmul_rn((double)x, stepX), fy = __dmul_rn((double)y, stepY);
    const int ix = (int)fx, iy = (int)fy;
    const int ix1 = ix + 1 < w - 1 ? ix + 1 : w - 1;
    const int iy1 = iy + 1 < h - 1 ? iy + 1 : h - 1;
    const double dx = __dsub_rn(fx, (double)ix), dy = __dsub_rn(fy, (double)iy);
    const double v00 = raw[(size_t)iy * w + ix], v01 = raw[(size_t)iy * w + ix1];
    const double v10 = raw[(size_t)iy1 * w + ix], v11 = raw[(size_t)iy1 * w + ix1];
    const double omdx = __dsub_rn(1.0, dx), omdy = __dsub_rn(1.0, dy);
    // (1-dx)*(1-dy)*v00 + dx*(1-dy)*v01 + (1-dx)*dy*v10 + dx*dy*v11, left to right, one rounding per operation
    double v = __dmul_rn(__dmul_rn(omdx, omdy), v00);
    v = __dadd_rn(v, __dmul_rn(__dmul_rn(dx, omdy), v01));
    v = __dadd_rn(v, __dmul_rn(__dmul_rn(omdx, dy), v10));
    v = __dadd_rn(v, __dmul_rn(__dmul_rn(dx, dy), v11));
    if constexpr (WINDOW) v = v < lo8 ? lo8 : v > hi8 ? hi8 : v;
    const double q = __dadd_rn(__dmul_rn(__dsub_rn(v, lo8), scale8), 0.5);
    dst[((size_t)y * outW + x) * dst_stride] = (uint8_t)(int)q;      // dst_stride > 1: one plane of an interleaved (HWC) tile
}

hipError_t launch_resample_u8(const uint16_t *raw, int w, int h, const unsigned *mnmx, uint8_t *dst, int outW, int outH,
                              int dst_stride, hipStream_t s)
{
    if (w <= 0 || h <= 0 || outW <= 0 || outH <= 0 || dst_stride < 1) return hipErrorInvalidValue;
    hipLaunchKernelGGL(resample_u8_kernel<false>, dim3((outW + 63) / 64, (outH + 3) / 4), dim3(256), 0, s, raw, w, h, mnmx, 0, 0, dst, outW,
                       outH, dst_stride);
    return hipGetLastError();
}

hipError_t launch_resample_u8_window(const uint16_t *raw, int w, int h, const unsigned *mnmx, int lo, int hi, uint8_t *dst, int outW,
                                     int outH, int dst_stride, hipStream_t s)
{
    if (w <= 0 || h <= 0 || outW <= 0 || outH <= 0 || dst_stride < 1) return hipErrorInvalidValue;
    if (!mnmx && (lo < 0 || lo > hi || hi > 65535)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(resample_u8_kernel<true>, dim3((outW + 63) / 64, (outH + 3) / 4), dim3(256), 0, s, raw, w, h, mnmx, lo, hi, dst, outW,
                       outH, dst_stride);
    return hipGetLastError();
}

// --------------------------------------------------------------------------------------------------------------------
// Intensity windows: the two order statistics of a plane by a two-pass radix select.  One 65536-bin histogram
// would need global atomics (256 KiB of u32 bins do not fit the LDS), and medical images pile onto a few hundred values: every
// wave of the plane would queue on the same words (see cc_stats below).  Instead: pass 1 counts the HIGH bytes -- 256 bins, one
// private histogram per wave in LDS, a lane merging the equal neighbours among its 8 samples before it touches LDS, the four waves
// summed in LDS and one global add per NON-EMPTY bin per workgroup; the head of pass 2 finds the two high bytes that hold the ranks
// (every workgroup scans the same 256 counts) and counts the LOW bytes of the samples under either; a one-workgroup kernel scans
// again and writes the pair.  No host round trip; the plane is read twice.
struct WindowScratch {
    unsigned hi_hist[256];          // samples per high byte
    unsigned lo_hist[2][256];       // samples per low byte under the high byte of rank 0 / of rank 1 (unused when both share one)
};
constexpr unsigned WIN_NONE = 0xFFFFFFFFu;

// The bin of hist[256] that holds rank k (cum(b - 1) <= k < cum(b)) and k - cum(b - 1), for two ranks at once; all 256 threads
// call it and all receive the result.  Counts sum to < 2^32.
struct WindowPick { unsigned bin[2], rest[2]; };
__device__ __forceinline__ WindowPick window_pick2(const unsigned *hist, unsigned k0, unsigned k1, unsigned *s_tot /*[4]*/,
                                                   unsigned *s_sel /*[4]*/)
{
    const unsigned t = threadIdx.x, c = hist[t];
    unsigned inc = c;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {                          // inclusive scan inside the wave
        const unsigned u = (unsigned)__shfl_up((int)inc, o, 64);
        if ((t & 63) >= (unsigned)o) inc += u;
    }
    if (t < 4) s_sel[t] = 0;
    if ((t & 63) == 63) s_tot[t >> 6] = inc;
    __syncthreads();
    for (unsigned wv = 0; wv < (t >> 6); ++wv) inc += s_tot[wv];
    const unsigned exc = inc - c;
    if (exc <= k0 && k0 < inc) { s_sel[0] = t; s_sel[1] = k0 - exc; }      // exactly one non-empty bin per rank
    if (exc <= k1 && k1 < inc) { s_sel[2] = t; s_sel[3] = k1 - exc; }
    __syncthreads();
    const WindowPick p{ { s_sel[0], s_sel[2] }, { s_sel[1], s_sel[3] } };
    __syncthreads();                                            // s_tot / s_sel may be reused
    return p;
}

// LOW = false: pass 1, hi_hist += high bytes.  LOW = true: pass 2, lo_hist[j] += low bytes of the samples whose high byte holds rank j.
template <bool LOW>
__global__ __launch_bounds__(256) void window_hist_kernel(const uint16_t *__restrict__ raw, size_t n, WindowScratch *ws, unsigned k0,
                                                          unsigned k1)
{
    constexpr int NH = LOW ? 2 : 1;
    __shared__ unsigned s_h[4][NH * 256];
    __shared__ unsigned s_tot[4], s_sel[4];
    for (int i = threadIdx.x; i < 4 * NH * 256; i += 256) (&s_h[0][0])[i] = 0;
    unsigned hb0 = 0, hb1 = 0;
    if constexpr (LOW) {
        const WindowPick p = window_pick2(ws->hi_hist, k0, k1, s_tot, s_sel);
        hb0 = p.bin[0]; hb1 = p.bin[1];
    }
    __syncthreads();
    unsigned *mine = s_h[threadIdx.x >> 6];
    unsigned cur = WIN_NONE, cnt = 0;                           // a lane's run of equal keys: one LDS add per run
    auto put = [&](unsigned v) {
        unsigned key;
        if constexpr (LOW) key = (v >> 8) == hb0 ? (v & 255u) : (v >> 8) == hb1 ? 256u + (v & 255u) : WIN_NONE;
        else key = v >> 8;
        if (key != cur) {
            if (cnt) atomicAdd(&mine[cur], cnt);
            cur = key; cnt = 0;
        }
        cnt += key != WIN_NONE;                                 // cnt > 0 only under a real key
    };
    const size_t n8 = n / 8, stride = (size_t)gridDim.x * 256;  // 16 bytes = 8 samples per lane, four loads in flight
    const uint4 *v = reinterpret_cast<const uint4 *>(raw);
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n8; i += 4 * stride) {
        uint4 q[4];
#pragma unroll
        for (int u = 0; u < 4; ++u)
            if (i + u * stride < n8) q[u] = v[i + u * stride];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            if (i + u * stride >= n8) break;
            const unsigned wd[4] = { q[u].x, q[u].y, q[u].z, q[u].w };
#pragma unroll
            for (int k = 0; k < 4; ++k) { put(wd[k] & 0xFFFFu); put(wd[k] >> 16); }
        }
    }
    if (blockIdx.x == 0 && threadIdx.x < (n & 7)) put(raw[n8 * 8 + threadIdx.x]);       // ragged tail
    if (cnt) atomicAdd(&mine[cur], cnt);
    __syncthreads();
    const int used = (LOW && hb0 != hb1) ? 2 : 1;
    for (int j = 0; j < used; ++j) {
        const int b = j * 256 + threadIdx.x;
        const unsigned sum = s_h[0][b] + s_h[1][b] + s_h[2][b] + s_h[3][b];
        if (sum) atomicAdd(LOW ? &ws->lo_hist[j][threadIdx.x] : &ws->hi_hist[threadIdx.x], sum);
    }
}

__global__ __launch_bounds__(256) void window_pick_kernel(const WindowScratch *ws, unsigned k0, unsigned k1, unsigned *mnmx)
{
    __shared__ unsigned s_tot[4], s_sel[4];
    const WindowPick hi = window_pick2(ws->hi_hist, k0, k1, s_tot, s_sel);
    const bool one = hi.bin[0] == hi.bin[1];                    // both ranks under one high byte: one low-byte histogram serves both
    const WindowPick a = window_pick2(ws->lo_hist[0], hi.rest[0], one ? hi.rest[1] : hi.rest[0], s_tot, s_sel);
    unsigned low1 = a.bin[1];
    if (!one) low1 = window_pick2(ws->lo_hist[1], hi.rest[1], hi.rest[1], s_tot, s_sel).bin[0];
    if (threadIdx.x == 0) {
        mnmx[0] = (hi.bin[0] << 8) | a.bin[0];
        mnmx[1] = (hi.bin[1] << 8) | low1;
    }
}

size_t window_scratch_bytes() { return sizeof(WindowScratch); }

hipError_t launch_window_select_u16(const uint16_t *raw, size_t n, int clip_lo_ppm, int clip_hi_ppm, void *scratch, unsigned *mnmx,
                                    hipStream_t s)
{
    if (!raw || !scratch || !mnmx || n == 0 || n >= (1ull << 32) || (reinterpret_cast<uintptr_t>(raw) & 15)) return hipErrorInvalidValue;
    if (clip_lo_ppm < 0 || clip_hi_ppm < 0 || (long long)clip_lo_ppm + clip_hi_ppm >= 1000000) return hipErrorInvalidValue;
    // ranks in 64-bit integers: n < 2^32, ppm < 2^20.  k_lo + k_hi <= n - 1, so k0 <= k1
    const unsigned k0 = (unsigned)((unsigned long long)n * (unsigned)clip_lo_ppm / 1000000ull);
    const unsigned k1 = (unsigned)(n - 1 - (unsigned long long)n * (unsigned)clip_hi_ppm / 1000000ull);
    size_t blocks = (n / 8 + 1023) / 1024;                      // four vectors per lane and trip
    if (blocks > 512) blocks = 512;
    if (blocks == 0) blocks = 1;
    WindowScratch *ws = static_cast<WindowScratch *>(scratch);
    hipLaunchKernelGGL(window_hist_kernel<false>, dim3((unsigned)blocks), dim3(256), 0, s, raw, n, ws, k0, k1);
    hipLaunchKernelGGL(window_hist_kernel<true>, dim3((unsigned)blocks), dim3(256), 0, s, raw, n, ws, k0, k1);
    hipLaunchKernelGGL(window_pick_kernel, dim3(1), dim3(256), 0, s, ws, k0, k1, mnmx);
    return hipGetLastError();
}

// --------------------------------------------------------------------------------------------------------------------
// postprocess_mask on the device.  Byte/integer work, HBM/L2-bound and tiny next to the network:
// the point is to keep the label maps on the device and to replace the reference's O(components x H x W) loops
// (src/postprocess.cpp:41, :71) by one union-find labelling.
namespace pp {

// fg[i] != 0 marks foreground.  parent = first pixel of the horizontal run inside the lane's 64-pixel segment (so the
// forest starts with chains no longer than W/64 per row instead of one node per pixel), -1 for background; stats cleared.
__global__ __launch_bounds__(256) void cc_init(const uint8_t *__restrict__ fg, int *parent, int *area, int *minx, int *miny,
                                               int *maxx, int *maxy, int W, long long n)
{
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    const bool in = i < n;
    const bool f = in && fg[i] != 0;
    const int x = in ? (int)(i % W) : 0;
    const int lane = threadIdx.x & 63;
    const unsigned long long fm = __ballot(f);
    const unsigned long long prev = (fm << 1) & ~__ballot(x == 0);      // lanes whose left neighbour (same row, same wave) is fg
    const unsigned long long starts = fm & ~prev;                        // first pixel of each run in this segment
    if (in) {
        int p = -1;
        if (f) {
            const unsigned long long below = starts & ((2ull << lane) - 1ull);
            p = (int)i - (lane - (63 - __builtin_clzll(below)));
        }
        parent[i] = p;
        area[i] = 0; minx[i] = 0x7FFFFFFF; miny[i] = 0x7FFFFFFF; maxx[i] = -1; maxy[i] = -1;
    }
}

// 8-connected unions.  Horizontal: only where a run continues across a 64-pixel segment boundary.  Vertical: with the
// pixel above if it is set -- skipped when the left neighbour and the upper-left pixel are set too (that pair already made
// the same connection) -- otherwise with the two upper diagonals.
__global__ __launch_bounds__(256) void cc_merge(const uint8_t *__restrict__ fg, int *parent, int H, int W, long long n)
{
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n || !fg[i]) return;
    const int hw = H * W;
    const int p = (int)(i % hw), y = p / W, x = p - y * W;
    const bool l = x > 0 && fg[i - 1];
    if (l && (threadIdx.x & 63) == 0) unite(parent, (int)i, (int)i - 1);
    if (y > 0) {
        const bool ul = x > 0 && fg[i - W - 1], u = fg[i - W] != 0, ur = x + 1 < W && fg[i - W + 1];
        if (u) {
            if (!(l && ul)) unite(parent, (int)i, (int)i - W);
        } else {
            if (ul && !l) unite(parent, (int)i, (int)i - W - 1);      // with l set, the left pixel makes this union (as its 'u' or 'ur')
            if (ur) unite(parent, (int)i, (int)i - W + 1);
        }
    }
}

// flatten + per-component area and bounding box.  Lanes of a wave mostly share one root, and same-address atomics serialise
// (a mask is a handful of components: every wave of the image would queue on the same five words -- 0.25 ms per call at
// 4 x 1024^2, profiles/r04_image_stage_kernels.txt), so a wave reduces per distinct root inside a 64-pixel segment AND carries
// that root's sums over CC_RUN consecutive segments, issuing the five atomics only when the root changes.
constexpr int CC_RUN = 16;
__global__ __launch_bounds__(256) void cc_stats(int *parent, int *area, int *minx, int *miny, int *maxx, int *maxy, int H, int W,
                                                long long n)
{
    const int lane = threadIdx.x & 63;
    const long long first = (((long long)blockIdx.x * 256 + threadIdx.x) >> 6) * (64LL * CC_RUN);
    int ar = -1, an = 0, alx = 0x7FFFFFFF, ahx = -1, aly = 0x7FFFFFFF, ahy = -1;      // the carried root and its sums (wave-uniform)
    auto flush = [&]() {
        if (ar >= 0 && lane == 0) {
            atomicAdd(area + ar, an);
            atomicMin(minx + ar, alx); atomicMax(maxx + ar, ahx);
            atomicMin(miny + ar, aly); atomicMax(maxy + ar, ahy);
        }
    };
    for (int sg = 0; sg < CC_RUN; ++sg) {
        const long long i = first + 64LL * sg + lane;
        if (first + 64LL * sg >= n) break;                          // (wave-uniform)
        int r = -1, x = 0, y = 0;
        if (i < n && parent[i] >= 0) {
            r = find_root_ro(parent, (int)i);
            parent[i] = r;
            const int p = (int)(i % ((long long)H * W));
            y = p / W; x = p - y * W;
        }
        wave::peel<64>(r, -1, [&](int r0, bool mine, unsigned long long m, int) {
            const int lx = wave::wave_min(mine ? x : 0x7FFFFFFF), hx = wave::wave_max(mine ? x : -1);
            const int ly = wave::wave_min(mine ? y : 0x7FFFFFFF), hy = wave::wave_max(mine ? y : -1);
            if (r0 != ar) { flush(); ar = r0; an = 0; alx = 0x7FFFFFFF; ahx = -1; aly = 0x7FFFFFFF; ahy = -1; }
            an += __builtin_popcountll(m);
            alx = min(alx, lx); ahx = max(ahx, hx); aly = min(aly, ly); ahy = max(ahy, hy);
        });
    }
    flush();
}

template <bool DILATE>
__global__ __launch_bounds__(256) void k_morph3(const uint8_t *__restrict__ src, uint8_t *dst, int H, int W, long long n)
{
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const int hw = H * W;
    const int p = (int)(i % hw), y = p / W, x = p - y * W;
    unsigned v = DILATE ? 0u : 255u;
#pragma unroll
    for (int dy = -1; dy <= 1; ++dy)
#pragma unroll
        for (int dx = -1; dx <= 1; ++dx) {
            const int yy = y + dy, xx = x + dx;
            if (yy < 0 || yy >= H || xx < 0 || xx >= W) continue;          // the border never constrains / never seeds
            const unsigned sv = src[i + dy * W + dx];
            v = DILATE ? max(v, sv) : min(v, sv);
        }
    dst[i] = (uint8_t)v;
}

// ---- the three kernels that look at a class or an area bound.  Plane p = i / hw of the output is target p % K of image p / K; they
// read the label map of the plane's image in place.  The table is a kernel argument; its entries are picked with a chain of
// selects, so it stays in registers.  The reference's single target is the table { 1, { 2 }, { min_area } }.
struct PlaneTarget { int cls, min_area; long long src; };
__device__ __forceinline__ PlaneTarget plane_target(const TargetTable &t, long long i, int hw)
{
    const int p = (int)((unsigned)i / (unsigned)hw), img = p / t.K, k = p - img * t.K;      // i < n <= 2^31 - 1
    int c = t.cls[0], a = t.min_area[0];
#pragma unroll
    for (int j = 1; j < POSTPROCESS_MAX_TARGETS; ++j)
        if (k == j) { c = t.cls[j]; a = t.min_area[j]; }
    return { c, a, (long long)img * hw + (i - (long long)p * hw) };
}

__global__ __launch_bounds__(256) void k_inv_multi(const uint8_t *__restrict__ labels, uint8_t *inv, int hw, TargetTable t, long long n)
{
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const PlaneTarget pt = plane_target(t, i, hw);
    inv[i] = labels[pt.src] == pt.cls ? 0 : 255;               // src/postprocess.cpp:18-22
}

// bin = 255 where the pixel is foreground after hole filling (src/postprocess.cpp:30-43, :57)
__global__ __launch_bounds__(256) void k_fill_bin_multi(const uint8_t *__restrict__ labels, const int *__restrict__ parent,
                                                        const int *__restrict__ area, const int *__restrict__ minx,
                                                        const int *__restrict__ miny, const int *__restrict__ maxx,
                                                        const int *__restrict__ maxy, uint8_t *bin, int H, int W, TargetTable t, long long n)
{
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const PlaneTarget pt = plane_target(t, i, H * W);
    bool fgd = labels[pt.src] == pt.cls;
    const int r = parent[i];
    if (!fgd && r >= 0)
        fgd = minx[r] > 0 && miny[r] > 0 && maxx[r] < W - 1 && maxy[r] < H - 1 && area[r] < pt.min_area;
    bin[i] = fgd ? 255 : 0;
}

__global__ __launch_bounds__(256) void k_filter_multi(const int *__restrict__ parent, const int *__restrict__ area, uint8_t *out, int hw,
                                                      TargetTable t, long long n)
{
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const PlaneTarget pt = plane_target(t, i, hw);
    const int r = parent[i];
    out[i] = (r >= 0 && area[r] >= pt.min_area) ? (uint8_t)pt.cls : 0;      // src/postprocess.cpp:70, :75-76
}

}  // namespace pp

size_t postprocess_workspace_bytes(int B, int H, int W)
{
    const size_t n = (size_t)B * H * W;
    return n * (6 * sizeof(int) + 3);                           // parent, area, 4 x bbox, three u8 planes
}

hipError_t launch_postprocess_masks_multi(const uint8_t *labels, uint8_t *out, int B, int H, int W, const TargetTable &t, void *ws,
                                          hipStream_t s)
{
    if (t.K < 1 || t.K > POSTPROCESS_MAX_TARGETS || B <= 0 || H <= 0 || W <= 0) return hipErrorInvalidValue;
    const long long n = (long long)B * t.K * H * W;                // the planes of all (image, target) pairs
    if (n <= 0 || n > 0x7FFFFFFFLL) return hipErrorInvalidValue;
    const int hw = H * W;
    // `out` may be the label map itself when K == 1: k_filter_multi reads no labels, and every read of them is ordered before it on
    // `s`.  With K > 1 the planes of image b would overwrite the label maps of the images behind it.
    const uintptr_t l0 = reinterpret_cast<uintptr_t>(labels), o0 = reinterpret_cast<uintptr_t>(out);
    if (t.K > 1 && o0 < l0 + (uintptr_t)B * hw && l0 < o0 + (uintptr_t)n) return hipErrorInvalidValue;
    int *parent = static_cast<int *>(ws), *area = parent + n, *minx = area + n, *miny = minx + n, *maxx = miny + n, *maxy = maxx + n;
    uint8_t *u0 = reinterpret_cast<uint8_t *>(maxy + n), *u1 = u0 + n, *u2 = u1 + n;
    const dim3 g((unsigned)((n + 255) / 256)), b(256);
    auto label = [&](const uint8_t *fg) {
        hipLaunchKernelGGL(pp::cc_init, g, b, 0, s, fg, parent, area, minx, miny, maxx, maxy, W, n);
        hipLaunchKernelGGL(pp::cc_merge, g, b, 0, s, fg, parent, H, W, n);
        hipLaunchKernelGGL(pp::cc_stats, dim3((unsigned)((n + 256LL * pp::CC_RUN - 1) / (256LL * pp::CC_RUN))), b, 0, s, parent, area, minx, miny, maxx, maxy, H, W, n);
    };
    hipLaunchKernelGGL(pp::k_inv_multi, g, b, 0, s, labels, u0, hw, t, n);
    label(u0);
    hipLaunchKernelGGL(pp::k_fill_bin_multi, g, b, 0, s, labels, parent, area, minx, miny, maxx, maxy, u1, H, W, t, n);
    uint8_t *opened = u1;
    if (morph_is_default(t)) {
        hipLaunchKernelGGL(pp::k_morph3<false>, g, b, 0, s, u1, u2, H, W, n);
        hipLaunchKernelGGL(pp::k_morph3<true>, g, b, 0, s, u2, u1, H, W, n);
    } else {                                                    // a target's own element (mi_unet_set_morph): between u1 and u2
        if (hipError_t e = launch_morph_chain(u1, u2, B * t.K, H, W, t, &opened, s); e != hipSuccess) return e;
    }
    label(opened);
    hipLaunchKernelGGL(pp::k_filter_multi, g, b, 0, s, parent, area, out, hw, t, n);
    return hipGetLastError();
}

// --------------------------------------------------------------------------------------------------------------------
// extract_contours on the device.
// OpenCV's sequential Suzuki-Abe scan interleaves "find the next start pixel" with "follow that border".  For
// RETR_EXTERNAL both halves separate cleanly:
//   * the start pixel of a component's outer border is its first pixel in raster order = the ROOT of the union-find
//     labelling above (parents always point to smaller indices);
//   * the border is external iff the background region just above that pixel reaches the image frame (OpenCV's
//     `img0[lnbd] > 0` test says the same thing through the sign of the last border label on the row): the pixel above
//     the root is background by construction, and a 4-connected background component reaches the frame iff its
//     bounding box touches the image edge;
//   * the trace itself (first neighbour clockwise from west, then counter-clockwise from the arrival direction, a point
//     wherever the step direction changes) is inherently serial per contour, so every external contour gets its own
//     lane: contours and images run in parallel, the mask is L2-resident (256 KB per image);
//   * OpenCV returns contours newest-first = descending raster order of the start pixels: a 64-bit-free trick -- the
//     per-image list of external roots is sorted by one thread per image (a handful of entries after postprocess_mask).
namespace ct {

__global__ __launch_bounds__(256) void k_threshold(const uint8_t *__restrict__ mask, uint8_t *fg, uint8_t *bg, long long n)
{
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const bool f = mask[i] > 127;                               // cv::threshold(127, 255, THRESH_BINARY)
    fg[i] = f ? 255 : 0;
    bg[i] = f ? 0 : 255;
}

// 4-connected unions (background regions): across segment boundaries horizontally; vertically unless the left pair
// already made the connection
__global__ __launch_bounds__(256) void cc_merge4(const uint8_t *__restrict__ fg, int *parent, int H, int W, long long n)
{
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n || !fg[i]) return;
    const int hw = H * W;
    const int p = (int)(i % hw), y = p / W, x = p - y * W;
    const bool l = x > 0 && fg[i - 1];
    if (l && (threadIdx.x & 63) == 0) pp::unite(parent, (int)i, (int)i - 1);
    if (y > 0 && fg[i - W] && !(l && fg[i - W - 1])) pp::unite(parent, (int)i, (int)i - W);
}

__global__ __launch_bounds__(256) void k_zero_counts(int *counts, int B)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < B) counts[i] = 0;
}

// a background component reaches the image frame iff one of the frame's pixels belongs to it: every background pixel of the frame
// flags its root (`flag`: zeroed by cc_init).  2 (H + W) pixels per image instead of a statistics pass over all of them.
__global__ __launch_bounds__(256) void k_frame_flags(const int *__restrict__ bparent, int *flag, int H, int W, int B)
{
    const int per = 2 * (H + W), t = blockIdx.x * 256 + threadIdx.x;
    if (t >= B * per) return;
    const int img = t / per, k = t - img * per;
    const int y = k < W ? 0 : k < 2 * W ? H - 1 : k < 2 * W + H ? k - 2 * W : k - 2 * W - H;
    const int x = k < W ? k : k < 2 * W ? k - W : k < 2 * W + H ? 0 : W - 1;
    const int p = img * H * W + y * W + x;
    if (bparent[p] >= 0) flag[pp::find_root_ro(bparent, p)] = 1;
}

// one entry per external component: its root (= start pixel).  fparent: fg labelling (not flattened: only `is a root` is asked);
// bparent + flag: background labelling (not flattened either) and which of its roots reach the frame.
__global__ __launch_bounds__(256) void k_collect(const int *__restrict__ fparent, const int *__restrict__ bparent,
                                                 const int *__restrict__ flag, int *roots, int *counts, int cap, int H, int W, long long n)
{
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n || fparent[i] != (int)i) return;                // roots only
    const int hw = H * W, img = (int)(i / hw);
    const int p = (int)(i % hw), y = p / W;
    bool external = (y == 0);
    if (!external)                                              // the pixel above a component's first pixel is background
        external = bparent[i - W] >= 0 && flag[pp::find_root_ro(bparent, (int)(i - W))] != 0;
    if (external) {
        const int slot = atomicAdd(counts + img, 1);
        if (slot < cap) roots[(size_t)img * cap + slot] = p;
    }
}

// per image: sort the start pixels descending (newest contour first).  Few entries: insertion sort by one lane.
__global__ __launch_bounds__(64) void k_sort_roots(int *roots, const int *counts, int cap, int B)
{
    const int img = blockIdx.x * 64 + threadIdx.x;
    if (img >= B) return;
    const int n = counts[img] < cap ? counts[img] : cap;
    int *r = roots + (size_t)img * cap;
    for (int a = 1; a < n; ++a) {
        const int v = r[a];
        int b = a - 1;
        while (b >= 0 && r[b] < v) { r[b + 1] = r[b]; --b; }
        r[b + 1] = v;
    }
}

// one lane per (image, contour): follow the border from its start pixel, emit CHAIN_APPROX_SIMPLE points.
// pass 0 counts points (npts) -- and already WRITES contour 0, whose offset is 0 whatever the counts are; pass 1 writes the
// others at the offsets computed in between and returns at once for images with a single contour (the usual case behind
// postprocess_mask, which keeps components of at least 6 % of the tile).
// The walk is a chain of dependent pixel probes (2-8 per border step), so the probe latency IS the kernel time: a workgroup
// = one image first packs the thresholded mask into an LDS bit plane (H*W/8 bytes: 32 KB at 512x512; images past the LDS
// budget keep probing global memory), then the lanes that own a contour walk it at LDS latency.
// PAD (IN_LDS and W % 32 == 0, so that rows are whole words): the plane carries one zero row above the image and one below it.
// Every row of a 3 x 3 probe then exists, the window's first bit is never negative, and the three rows of a probe share their
// shift -- the probe of a border step loses its row tests and selects.
template <bool IN_LDS, bool PAD = false>
__global__ __launch_bounds__(256) void k_trace(const uint8_t *__restrict__ fg, const int *__restrict__ roots,
                                               const int *__restrict__ counts, int cap, int H, int W, int B, int *npts,
                                               const int *__restrict__ offs, int *out_xy, int cap_points, int write)
{
    extern __shared__ unsigned bits[];
    const int img = blockIdx.x;
    const uint8_t *im = fg + (size_t)img * H * W;
    const int nc = counts[img];
    if (nc <= 0 || nc > cap) return;                             // workgroup-uniform
    if (write && nc == 1) return;                                // contour 0 was written by the count pass
    static_assert(!PAD || IN_LDS, "the padded plane lives in LDS");
    const int padw = PAD ? (W >> 5) : 0;                         // words of the zero row in front of the image
    if constexpr (IN_LDS) {
        const int nwords = (H * W + 31) >> 5;
        if (threadIdx.x == 0) bits[nwords + 2 * padw] = 0;       // one word past the plane: the 64-bit windows below may touch it
        if constexpr (PAD)
            for (int w = threadIdx.x; w < padw; w += 256) { bits[w] = 0; bits[padw + nwords + w] = 0; }
        for (int w = threadIdx.x; w < nwords; w += 256) {
            unsigned m = 0;
            const int base = w << 5;
            if (base + 32 <= H * W && (((uintptr_t)(im + base)) & 15) == 0) {
                const uint4 q0 = *reinterpret_cast<const uint4 *>(im + base), q1 = *reinterpret_cast<const uint4 *>(im + base + 16);
                const unsigned ws[8] = { q0.x, q0.y, q0.z, q0.w, q1.x, q1.y, q1.z, q1.w };
#pragma unroll
                for (int k = 0; k < 8; ++k)
#pragma unroll
                    for (int b4 = 0; b4 < 4; ++b4) m |= (((ws[k] >> (8 * b4)) & 0xFFu) != 0 ? 1u : 0u) << (4 * k + b4);
            } else {
                for (int k = 0; k < 32 && base + k < H * W; ++k) m |= (im[base + k] != 0 ? 1u : 0u) << k;
            }
            bits[padw + w] = m;
        }
        __syncthreads();
    }
    auto at = [&](int x, int y) -> bool {
        if (x < 0 || x >= W || y < 0 || y >= H) return false;
        const int p = y * W + x;
        if constexpr (IN_LDS) return (bits[padw + (p >> 5)] >> (p & 31)) & 1u;
        else return im[p] != 0;
    };
    // direction d: 0 = E, then counter-clockwise on screen (y grows down): DX = {1,1,0,-1,-1,-1,0,1}, DY = {0,-1,-1,-1,0,1,1,1}.
    // Packed as nibbles of (value + 1): a dynamically indexed array would live in scratch memory, and every probe of the walk
    // would pay a memory round trip for its offsets.
    auto DX = [](int d) -> int { return (int)((0x21000122u >> (4 * d)) & 3u) - 1; };
    auto DY = [](int d) -> int { return (int)((0x22210001u >> (4 * d)) & 3u) - 1; };
    for (int c = threadIdx.x; c < nc; c += 256) {               // lanes own contours (a handful after postprocess_mask)
    if (write && c == 0) continue;                               // written by the count pass
    const int start = roots[(size_t)img * cap + c];
    const int x0 = start % W, y0 = start / W;
    int *dst = nullptr;
    int room = 0;
    const bool store = write || c == 0;
    if (store) {
        const int o = write ? offs[(size_t)img * (cap + 1) + c] : 0;
        room = cap_points - o;
        dst = out_xy + ((size_t)img * cap_points + o) * 2;
    }
    int n = 0;
    auto emit = [&](int x, int y) {
        if (store && n < room) { dst[2 * n] = x; dst[2 * n + 1] = y; }
        ++n;
    };
    // The walk is a chain of dependent steps; inside a step the eight neighbour probes are INDEPENDENT reads (issued together,
    // one LDS latency), and the search order -- counter-clockwise from the arrival direction -- is a rotate + find-first-set
    // on the resulting 8-bit mask instead of up to eight chained probes.
    // three pixels (x-1, x, x+1) of row y as bits 0..2: the rows of the plane are packed back to back, so they are three
    // CONSECUTIVE bits of one 64-bit window (two LDS words), whatever W is; columns outside the image are masked off
    // Branch-free: a row outside the image reads the plane's first words and is masked to zero afterwards, so the six LDS reads of a
    // step are issued together and waited for ONCE (with an early return per row hipcc waited three times per border pixel).
    auto nb8 = [&](int x, int y) -> unsigned {                  // bit d = neighbour in direction d is foreground
        if constexpr (PAD) {
            const unsigned cols = (x > 0 ? 7u : 6u) & (x + 1 < W ? 7u : 3u);
            const int q = (y + 1) * W + x - 1;                  // row y of the image is row y + 1 of the plane: q >= W - 1
            const unsigned *const b = bits + (q >> 5);
            const int sh = q & 31;
            unsigned r[3];
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                const unsigned *const bk = b + (k - 1) * padw;
                r[k] = (unsigned)((((unsigned long long)bk[1] << 32) | bk[0]) >> sh) & cols;
            }
            return ((r[1] >> 2) & 1u) | (((r[0] >> 2) & 1u) << 1) | (((r[0] >> 1) & 1u) << 2) | ((r[0] & 1u) << 3) | ((r[1] & 1u) << 4) |
                   ((r[2] & 1u) << 5) | (((r[2] >> 1) & 1u) << 6) | (((r[2] >> 2) & 1u) << 7);
        } else if constexpr (IN_LDS) {
            const unsigned cols = (x > 0 ? 7u : 6u) & (x + 1 < W ? 7u : 3u);
            unsigned r[3];
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                const int yy = y - 1 + k;
                const bool ok = (unsigned)yy < (unsigned)H;
                const int q = yy * W + x - 1;                   // first bit of the window; -1 only at the image origin
                const int qc = ok ? (q > 0 ? q : 0) : 0;
                const unsigned lo = bits[qc >> 5], hi = bits[(qc >> 5) + 1];
                unsigned v = (unsigned)((((unsigned long long)hi << 32) | lo) >> (qc & 31));
                if (q < 0) v <<= 1;
                r[k] = ok ? (v & cols) : 0u;
            }
            return ((r[1] >> 2) & 1u) | (((r[0] >> 2) & 1u) << 1) | (((r[0] >> 1) & 1u) << 2) | ((r[0] & 1u) << 3) | ((r[1] & 1u) << 4) |
                   ((r[2] & 1u) << 5) | (((r[2] >> 1) & 1u) << 6) | (((r[2] >> 2) & 1u) << 7);
        } else {
            unsigned m = 0;
#pragma unroll
            for (int d = 0; d < 8; ++d) m |= (at(x + DX(d), y + DY(d)) ? 1u : 0u) << d;
            return m;
        }
    };
    int first = -1;                                             // first neighbour: clockwise, starting after west
    {
        const unsigned m = nb8(x0, y0);
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            const int d = (3 - k) & 7;                          // 3, 2, 1, 0, 7, 6, 5, 4
            if (first < 0 && ((m >> d) & 1u)) first = d;
        }
    }
    if (first < 0) {
        emit(x0, y0);                                           // isolated pixel
    } else {
        const int x1 = x0 + DX(first), y1 = y0 + DY(first);
        int cx = x0, cy = y0, came = first, last_step = first ^ 4;
        for (long long guard = 0; guard < 4LL * H * W + 16; ++guard) {      // a border has at most 4 visits per pixel
            const unsigned m = nb8(cx, cy);
            if (m == 0) break;                                  // cannot happen on a border pixel; keeps the loop finite on bad input
            const int base = (came + 1) & 7;                    // search came+1, came+2, ... (counter-clockwise)
            const unsigned rot = ((m | (m << 8)) >> base) & 0xFFu;
            const int step = (base + __builtin_ctz(rot)) & 7;
            const int nx = cx + DX(step), ny = cy + DY(step);
            if (step != last_step) { emit(cx, cy); last_step = step; }
            const bool closing = (nx == x0 && ny == y0 && cx == x1 && cy == y1);
            cx = nx; cy = ny;
            if (closing) break;
            came = (step + 4) & 7;
        }
    }
    if (!write) npts[(size_t)img * cap + c] = n;
    }
}

// per image: exclusive scan of the point counts -> out_start, and the verdict (count or -1 on overflow)
__global__ __launch_bounds__(64) void k_offsets(const int *__restrict__ npts, const int *__restrict__ counts, int cap,
                                                int cap_points, int B, int *out_start, int *out_count)
{
    const int img = blockIdx.x * 64 + threadIdx.x;
    if (img >= B) return;
    int *st = out_start + (size_t)img * (cap + 1);
    const int nc = counts[img];
    if (nc > cap) { out_count[img] = -1; st[0] = 0; return; }
    int o = 0;
    for (int c = 0; c < nc; ++c) { st[c] = o; o += npts[(size_t)img * cap + c]; }
    st[nc] = o;
    out_count[img] = o > cap_points ? -1 : nc;
}

}  // namespace ct

__global__ __launch_bounds__(256) void mask_to_image_binary_kernel(const uint8_t *masks, uint8_t *vis, size_t n)
{
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n) vis[i] = masks[i] ? 255 : 0;
}

hipError_t launch_mask_to_image_binary(const uint8_t *masks, uint8_t *vis, size_t n, hipStream_t s)
{
    hipLaunchKernelGGL(mask_to_image_binary_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, masks, vis, n);
    return hipGetLastError();
}

size_t contour_workspace_bytes(int B, int H, int W, int cap_contours)
{
    const size_t n = (size_t)B * H * W;
    return n * (7 * sizeof(int) + 2) + sizeof(int) * ((size_t)B * (2 * cap_contours + 1) + 64);
}

// The labelling half: threshold, both forests, the external roots of every plane collected and sorted (contour order).  Shared by the
// contour trace below and the region measurement (regions.hip).
hipError_t launch_label_contours(const uint8_t *masks, int B, int H, int W, int cap_contours, void *ws, hipStream_t s)
{
    const long long n = (long long)B * H * W;
    if (n <= 0 || n > 0x7FFFFFFFLL || cap_contours <= 0) return hipErrorInvalidValue;
    const ContourWs w = contour_ws(ws, n, B, cap_contours);
    const dim3 g((unsigned)((n + 255) / 256)), b(256);
    hipLaunchKernelGGL(ct::k_threshold, g, b, 0, s, masks, w.fg, w.bg, n);
    // foreground labelling (8-connected): only its roots are asked for (no statistics pass, no flattening)
    hipLaunchKernelGGL(pp::cc_init, g, b, 0, s, w.fg, w.fparent, w.flag, w.slot, w.miny, w.maxx, w.maxy, W, n);
    hipLaunchKernelGGL(pp::cc_merge, g, b, 0, s, w.fg, w.fparent, H, W, n);
    // background labelling (4-connected); `flag` (zeroed by cc_init) becomes the reaches-the-frame flag of its roots
    hipLaunchKernelGGL(pp::cc_init, g, b, 0, s, w.bg, w.bparent, w.flag, w.slot, w.miny, w.maxx, w.maxy, W, n);
    hipLaunchKernelGGL(ct::cc_merge4, g, b, 0, s, w.bg, w.bparent, H, W, n);
    hipLaunchKernelGGL(ct::k_frame_flags, dim3((unsigned)((B * 2 * (H + W) + 255) / 256)), b, 0, s, w.bparent, w.flag, H, W, B);
    hipLaunchKernelGGL(ct::k_zero_counts, dim3((B + 255) / 256), b, 0, s, w.counts, B);
    hipLaunchKernelGGL(ct::k_collect, g, b, 0, s, w.fparent, w.bparent, w.flag, w.roots, w.counts, cap_contours, H, W, n);
    hipLaunchKernelGGL(ct::k_sort_roots, dim3((B + 63) / 64), dim3(64), 0, s, w.roots, w.counts, cap_contours, B);
    return hipGetLastError();
}

// The tracing half, behind launch_label_contours on the same workspace.
hipError_t launch_trace_contours(int B, int H, int W, int *out_xy, int cap_points, int *out_start, int cap_contours, int *out_count,
                                 void *ws, hipStream_t s)
{
    const long long n = (long long)B * H * W;
    if (n <= 0 || n > 0x7FFFFFFFLL || cap_contours <= 0 || cap_points <= 0) return hipErrorInvalidValue;
    const ContourWs w = contour_ws(ws, n, B, cap_contours);
    const uint8_t *fg = w.fg;
    int *roots = w.roots, *npts = w.npts, *counts = w.counts;
    // one workgroup per image; the mask as an LDS bit plane when it fits
    const size_t plane = (((size_t)H * W + 31) / 32) * 4 + 4;    // + one word of slack behind the plane (k_trace's windows)
    const bool in_lds = plane <= 160 * 1024;                     // the whole LDS of a CU: 1024x1024 is 128 KB + 4
    const size_t padded = plane + 2 * (size_t)(W / 32) * 4;      // + a zero row above and below (k_trace<true, true>)
    const bool pad = W % 32 == 0 && padded <= 160 * 1024;
    const dim3 gt((unsigned)B), bt(256);
    for (int pass = 0; pass < 2; ++pass) {
        if (pad) {
            if (hipError_t e = ensure_dynamic_lds(ct::k_trace<true, true>, padded); e != hipSuccess) return e;
            hipLaunchKernelGGL((ct::k_trace<true, true>), gt, bt, padded, s, fg, roots, counts, cap_contours, H, W, B, npts, out_start, out_xy, cap_points, pass);
        } else if (in_lds) {
            if (hipError_t e = ensure_dynamic_lds(ct::k_trace<true>, plane); e != hipSuccess) return e;
            hipLaunchKernelGGL(ct::k_trace<true>, gt, bt, plane, s, fg, roots, counts, cap_contours, H, W, B, npts, out_start, out_xy, cap_points, pass);
        } else {
            hipLaunchKernelGGL(ct::k_trace<false>, gt, bt, 0, s, fg, roots, counts, cap_contours, H, W, B, npts, out_start, out_xy, cap_points, pass);
        }
        if (pass == 0)
            hipLaunchKernelGGL(ct::k_offsets, dim3((B + 63) / 64), dim3(64), 0, s, npts, counts, cap_contours, cap_points, B, out_start, out_count);
    }
    return hipGetLastError();
}

hipError_t launch_extract_contours(const uint8_t *masks, int B, int H, int W, int *out_xy, int cap_points, int *out_start,
                                   int cap_contours, int *out_count, void *ws, hipStream_t s)
{
    if (cap_points <= 0) return hipErrorInvalidValue;
    if (hipError_t e = launch_label_contours(masks, B, H, W, cap_contours, ws, s); e != hipSuccess) return e;
    return launch_trace_contours(B, H, W, out_xy, cap_points, out_start, cap_contours, out_count, ws, s);
}


}  // namespace miunet
