// regions.hip -- region measurement (include/mi_unet.h: mi_unet_set_measure): area, bounding box, crack perimeter,
// raw moments and intensity sums of every contoured component, from what the contour stage leaves in device memory.  All integer,
// exact.  gfx950 only.
#include "../../include/mi_unet.h"
#include "cc_common.h"
#include "kernel_common.h"
#include "wave.h"

static_assert(sizeof(mi_unet_region) == 96, "mi_unet_region is 96 bytes without padding");
static_assert(offsetof(mi_unet_region, edges) == 32 && offsetof(mi_unet_region, sii) == 88, "mi_unet_region: eight ints, eight int64");

namespace miunet {
namespace rg {

using namespace wave;

// One thread per (plane, slot): the accumulator is the output struct itself.  A slot in use gets the identities of its min / max
// fields and its index written at the component's root in the slot map; every other entry -- behind the plane's count, and the whole
// plane when it holds more than `cap` external components -- is zero and stays zero (no pixel finds a slot there).
__global__ __launch_bounds__(256) void k_region_slots(const int *__restrict__ roots, const int *__restrict__ counts, int cap, int planes,
                                                      int hw, int *slot, mi_unet_region *regions, int *rcounts, int has_tiles,
                                                      int channel)
{
    const int t = blockIdx.x * 256 + threadIdx.x;
    if (t >= planes * cap) return;                              // planes * cap <= the roots array, which the workspace check bounds
    const int p = t / cap, c = t - p * cap;
    const int nc = counts[p];
    const bool fits = nc <= cap;
    if (c == 0) rcounts[p] = fits ? nc : -1;
    mi_unet_region r{};                                         // all-zero
    if (fits && c < nc) {
        r.x0 = 0x7FFFFFFF; r.y0 = 0x7FFFFFFF; r.x1 = -1; r.y1 = -1;
        r.imin = has_tiles ? 0x7FFFFFFF : 0;                    // without a tile every v is 0: min and max stay 0
        r.imax = has_tiles ? -1 : 0;
        r.channel = has_tiles ? channel : -1;
        slot[(size_t)p * hw + roots[t]] = c;                    // roots[p * cap + c] < hw: a pixel of the plane
    }
    regions[t] = r;
}

// One pass over the pixels of all planes.  A mask is a handful of components, so every wave of the image would queue on the same
// few structs (cc_stats, image_stages.hip): a wave reduces per distinct root inside a 64-pixel segment, carries that root's fifteen
// sums over RG_RUN consecutive segments and touches memory only when the root changes -- four atomic instructions per flush: eight
// lanes add the eight int64 sums (64 contiguous bytes), one the area, three take the minima, three the maxima.
// The forest is read as the contour path left it (not flattened): find_root_ro walks, nothing is stored.
constexpr int RG_RUN = 16;

template <bool TILES>
__global__ __launch_bounds__(256) void region_stats(const uint8_t *__restrict__ fg, const int *__restrict__ fparent,
                                                    const int *__restrict__ slot, const uint8_t *__restrict__ tiles, int in_ch,
                                                    int channel, int K, int H, int W, long long n, mi_unet_region *regions, int cap)
{
    const int lane = threadIdx.x & 63;
    const int hw = H * W;
    const long long first = (((long long)blockIdx.x * 256 + threadIdx.x) >> 6) * (64LL * RG_RUN);
    // the carried root and its sums (wave-uniform)
    int c_root = -1, c_area = 0, c_x0 = 0x7FFFFFFF, c_y0 = 0x7FFFFFFF, c_x1 = -1, c_y1 = -1, c_imin = 0x7FFFFFFF, c_imax = -1;
    long long c_edges = 0, c_sx = 0, c_sy = 0, c_sxx = 0, c_syy = 0, c_sxy = 0, c_si = 0, c_sii = 0;
    auto flush = [&]() __attribute__((always_inline)) {
        if (c_root < 0) return;                                 // (wave-uniform)
        const int c = slot[c_root];
        if (c == REGION_NO_SLOT) return;                        // no contour (nested in a hole) or a plane past its capacity
        mi_unet_region *const r = regions + (size_t)(c_root / hw) * cap + c;      // c < cap: written by k_region_slots
        // the value of lane k as an OR of masked terms: a chain of selects over the lane index becomes a table in scratch memory
        auto pick = [&](int k, long long v) -> long long { return lane == k ? v : 0; };
        auto pick32 = [&](int k, int v) -> int { return lane == k ? v : 0; };
        if (lane < 8) {
            const long long v = pick(0, c_edges) | pick(1, c_sx) | pick(2, c_sy) | pick(3, c_sxx) | pick(4, c_syy) | pick(5, c_sxy) |
                                pick(6, c_si) | pick(7, c_sii);
            atomicAdd(reinterpret_cast<unsigned long long *>(&r->edges) + lane, (unsigned long long)v);
        }
        if (lane == 0) atomicAdd(&r->area, c_area);
        if (lane < 3) {                                         // x0, y0, imin are ints 1, 2, 5 of the struct; x1, y1, imax 3, 4, 6
            int *const q = &r->area;
            atomicMin(q + 1 + lane + (lane == 2 ? 2 : 0), pick32(0, c_x0) | pick32(1, c_y0) | pick32(2, c_imin));
            atomicMax(q + 3 + lane + (lane == 2 ? 1 : 0), pick32(0, c_x1) | pick32(1, c_y1) | pick32(2, c_imax));
        }
    };
    for (int sg = 0; sg < RG_RUN; ++sg) {
        const long long base = first + 64LL * sg, i = base + lane;
        if (base >= n) break;                                   // (wave-uniform)
        int r = -1, x = 0, y = 0, v = 0, e = 0;
        if (i < n && fg[i]) {
            r = pp::find_root_ro(fparent, (int)i);
            const int pl = (int)(i / hw), p = (int)(i - (long long)pl * hw);
            y = p / W; x = p - y * W;
            // the four pixel edges towards something that is not foreground; the image frame counts as such
            e = (x == 0 || !fg[i - 1]) + (x == W - 1 || !fg[i + 1]) + (y == 0 || !fg[i - W]) + (y == H - 1 || !fg[i + W]);
            if constexpr (TILES) v = tiles[((size_t)(pl / K) * hw + p) * in_ch + channel];      // the plane's IMAGE: never replicated
        }
        peel<64>(r, -1, [&](int r0, bool mine, u64 m, int) {
            const long long lx = mine ? x : 0, ly = mine ? y : 0;
            const int pe = wave_sum(mine ? e : 0);
            const long long psx = wave_sum(lx), psy = wave_sum(ly), psxx = wave_sum(lx * lx), psyy = wave_sum(ly * ly),
                            psxy = wave_sum(lx * ly);
            const int px0 = wave_min(mine ? x : 0x7FFFFFFF), py0 = wave_min(mine ? y : 0x7FFFFFFF);
            const int px1 = wave_max(mine ? x : -1), py1 = wave_max(mine ? y : -1);
            if (r0 != c_root) {
                flush();
                c_root = r0; c_area = 0; c_x0 = 0x7FFFFFFF; c_y0 = 0x7FFFFFFF; c_x1 = -1; c_y1 = -1; c_imin = 0x7FFFFFFF; c_imax = -1;
                c_edges = 0; c_sx = 0; c_sy = 0; c_sxx = 0; c_syy = 0; c_sxy = 0; c_si = 0; c_sii = 0;
            }
            c_area += __builtin_popcountll(m);
            c_edges += pe; c_sx += psx; c_sy += psy; c_sxx += psxx; c_syy += psyy; c_sxy += psxy;
            c_x0 = min(c_x0, px0); c_y0 = min(c_y0, py0); c_x1 = max(c_x1, px1); c_y1 = max(c_y1, py1);
            if constexpr (TILES) {
                c_si += wave_sum(mine ? v : 0);                 // 64 * 255 and 64 * 255^2 fit an int
                c_sii += wave_sum(mine ? v * v : 0);
                c_imin = min(c_imin, wave_min(mine ? v : 0x7FFFFFFF));
                c_imax = max(c_imax, wave_max(mine ? v : -1));
            } else {
                c_imin = 0; c_imax = 0;                         // the identities of a slot without a tile (k_region_slots)
            }
        });
    }
    flush();
}

}  // namespace rg

hipError_t launch_measure_regions(int planes, int H, int W, int K, const uint8_t *tiles, int in_ch, int channel, mi_unet_region *regions,
                                  int *rcounts, int cap_contours, void *ws, hipStream_t s)
{
    const long long n = (long long)planes * H * W;
    if (n <= 0 || n > 0x7FFFFFFFLL || cap_contours <= 0 || K < 1 || planes % K != 0 || !regions || !rcounts || !ws)
        return hipErrorInvalidValue;
    if (tiles && (in_ch < 1 || channel < 0 || channel >= in_ch)) return hipErrorInvalidValue;
    if ((long long)planes * cap_contours > 0x7FFFFFFFLL) return hipErrorInvalidValue;
    const ContourWs w = contour_ws(ws, n, planes, cap_contours);
    const int slots = planes * cap_contours;
    hipLaunchKernelGGL(rg::k_region_slots, dim3((unsigned)((slots + 255) / 256)), dim3(256), 0, s, w.roots, w.counts, cap_contours, planes,
                       H * W, w.slot, regions, rcounts, tiles ? 1 : 0, channel);
    const dim3 g((unsigned)((n + 256LL * rg::RG_RUN - 1) / (256LL * rg::RG_RUN))), b(256);
    if (tiles)
        hipLaunchKernelGGL(rg::region_stats<true>, g, b, 0, s, w.fg, w.fparent, w.slot, tiles, in_ch, channel, K, H, W, n, regions, cap_contours);
    else
        hipLaunchKernelGGL(rg::region_stats<false>, g, b, 0, s, w.fg, w.fparent, w.slot, tiles, 1, 0, K, H, W, n, regions, cap_contours);
    return hipGetLastError();
}

}  // namespace miunet
