// volume_spatial.hip -- per component of a labelled stack its intensity sums, its intensity peaks and the inverse-distance pair sums
// behind Moran's I and Geary's C (include/mi_unet.h: mi_unet_volume_spatial).  k_vsp_sums: a lane per voxel, the wave
// reduces per distinct id and carries an id's sums until the id changes (the scheme of k_vms_sums).  k_vsp_prefix: a wave scan per row
// of the intensity.  k_vsp_fill: every voxel of a component into the component's segment with the sum and the count of its sphere, two
// prefix reads per row of the ball.  k_vsp_peaks: the best candidate of a segment, a workgroup per component.  k_vsp_rank and
// k_vsp_place: the points of a searched component in index order, so that the doubles below do not depend on the order of the fill.
// k_vsp_pairs, the hot path: an N-body tiling over the upper-triangular tile pairs of a segment, a point per lane against a tile in
// LDS, four double accumulators per lane, one slot of four doubles per work item.  No floating-point atomic; no workgroup waits for
// another.  gfx950 only.
#include "../../include/mi_unet.h"
#include "kernel_common.h"
#include "kernels.h"
#include "wave.h"

namespace miunet {

namespace vsp {

using namespace wave;

constexpr unsigned WG = 256;                // lanes per workgroup; = VSP_TILE in k_vsp_rank and k_vsp_pairs
constexpr int RUN = 16;                     // 64-voxel segments a wave of k_vsp_sums carries an id over
constexpr int GROUPS = 4;                   // distinct ids of a segment that are reduced across the wave; lanes beyond them add their own
constexpr int NONE = 0x7FFFFFFF;
constexpr int FIELDS = 11;                  // voxels, imin, imax and the eight sums
static_assert(VSP_TILE == (int)WG, "a lane per point of the a-tile, a lane per point of the b-tile's load");

// the sums of one id: n voxels, lo / hi of the intensity, sx, sy, sz, si, sii, six, siy, siz
struct Acc {
    int n, lo, hi;
    long long s[8];
};

// field f of the entry, 0 .. 10.  One atomic; a wave that holds the same acc in every lane issues eleven of them from eleven lanes at once.
// The sum is picked by selects: a run-time index would put acc into scratch.
__device__ __forceinline__ void add_field(mi_unet_vspatial *c, const Acc &a, int f)
{
    if (f == 0) atomicAdd(&c->voxels, a.n);
    else if (f == 1) atomicMax(&c->imin, 65535 - a.lo);         // (turned round by the caller: 0 = no voxel yet)
    else if (f == 2) atomicMax(&c->imax, a.hi);
    else {
        long long v = 0;
#pragma unroll
        for (int j = 0; j < 8; ++j) v = f - 3 == j ? a.s[j] : v;
        atomicAdd(reinterpret_cast<u64 *>(&c->sx) + (f - 3), (u64)v);
    }
}

// (x, y, z) of voxel i
__device__ __forceinline__ void coords(unsigned i, unsigned hw, int W, int &x, int &y, int &z)
{
    z = (int)(i / hw);
    const int rem = (int)(i - (unsigned)z * hw);
    y = rem / W;
    x = rem - y * W;
}

// ---- sums: one lane per voxel, consecutive lanes along x -------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_vsp_sums(const int32_t *__restrict__ ids, const uint16_t *__restrict__ inten, int H, int W,
                                                  unsigned dhw, int m, mi_unet_vspatial *table)
{
    const int lane = threadIdx.x & 63;
    const long long first = (((long long)blockIdx.x * WG + threadIdx.x) >> 6) * (64LL * RUN);
    const unsigned hw = (unsigned)H * (unsigned)W;
    int ar = -1;                                                // (wave-uniform) the id carried, and its sums
    Acc acc;
    auto reset = [&]() {
        acc.n = 0; acc.lo = 65535; acc.hi = 0;
#pragma unroll
        for (int j = 0; j < 8; ++j) acc.s[j] = 0;
    };
    auto flush = [&]() {
        if (ar >= 0 && lane < FIELDS) add_field(table + ar, acc, lane);
    };
    reset();
    for (int sg = 0; sg < RUN; ++sg) {
        if (first + 64LL * sg >= (long long)dhw) break;         // (wave-uniform)
        const long long i = first + 64LL * sg + lane;
        int r = -1, v = 0, x = 0, y = 0, z = 0;
        if (i < (long long)dhw) {
            const int id = ids[i];
            if (id >= 1 && id <= m) {
                r = id - 1;
                coords((unsigned)i, hw, W, x, y, z);
                v = inten[i];
            }
        }
        peel<GROUPS>(r, -1, [&](int r0, bool mine, u64 mm, int) {
            if (r0 != ar) {
                flush();
                reset();
                ar = r0;
            }
            acc.n += __popcll(mm);
            const long long cx = mine ? x : 0, cy = mine ? y : 0, cz = mine ? z : 0, cv = mine ? v : 0;
            acc.s[0] += wave_sum(cx); acc.s[1] += wave_sum(cy); acc.s[2] += wave_sum(cz);
            acc.s[3] += wave_sum(cv); acc.s[4] += wave_sum(cv * cv);
            acc.s[5] += wave_sum(cv * cx); acc.s[6] += wave_sum(cv * cy); acc.s[7] += wave_sum(cv * cz);
            acc.lo = min(acc.lo, wave_min(mine ? v : 65535));
            acc.hi = max(acc.hi, wave_max(mine ? v : 0));
        });
        if (r >= 0) {                                           // a segment of many small components: the lane adds its own voxel
            Acc one;
            one.n = 1; one.lo = v; one.hi = v;
            const long long cx = x, cy = y, cz = z, cv = v;
            one.s[0] = cx; one.s[1] = cy; one.s[2] = cz; one.s[3] = cv; one.s[4] = cv * cv;
            one.s[5] = cv * cx; one.s[6] = cv * cy; one.s[7] = cv * cz;
            for (int f = 0; f < FIELDS; ++f) add_field(table + r, one, f);
        }
    }
    flush();
}

// ---- prefix: a wave per row, 64 columns per step, the row's running sum carried -----------------------------------------------------------------
// prefix[row][k] = the sum of the row's first k intensities, 0 <= k <= W: below 8192 * 65535 < 2^29.
__global__ __launch_bounds__(256) void k_vsp_prefix(const uint16_t *__restrict__ inten, int W, unsigned rows, uint32_t *__restrict__ prefix)
{
    const unsigned row = blockIdx.x * 4u + (threadIdx.x >> 6);
    if (row >= rows) return;                                    // (wave-uniform)
    const int lane = threadIdx.x & 63;
    const uint16_t *const in = inten + (size_t)row * W;
    uint32_t *const out = prefix + (size_t)row * (W + 1);
    if (lane == 0) out[0] = 0;
    unsigned carry = 0;
    for (int x0 = 0; x0 < W; x0 += 64) {
        const int x = x0 + lane;
        unsigned v = x < W ? in[x] : 0u;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const unsigned t = (unsigned)__shfl_up((int)v, o, 64);
            if (lane >= o) v += t;
        }
        if (x < W) out[x + 1] = carry + v;
        carry += (unsigned)__shfl((int)v, 63, 64);
    }
}

// ---- fill: every voxel of a component into the component's segment, with its sphere -------------------------------------------------------------
// The sphere's sum is two prefix reads per row (dy, dz) of the ball that lies inside the volume, its count comes from the same clamped
// extents.  A wave takes one slot range per distinct id (one atomic each); the order inside a segment is that of arrival: the peaks are a
// maximum under a total order and k_vsp_place puts the points of the pair sums into index order.  A slot at or past the segment's size
// cannot occur while `voxels` is exact; it is dropped all the same.
__global__ __launch_bounds__(256) void k_vsp_fill(const int32_t *__restrict__ ids, const uint16_t *__restrict__ inten,
                                                  const uint32_t *__restrict__ prefix, VolumeSpatialArgs a, unsigned dhw,
                                                  const mi_unet_vspatial *__restrict__ table, const int4 *__restrict__ seg,
                                                  const int4 *__restrict__ rows, int n_rows, int *cursor, VspCand *__restrict__ cand)
{
    const unsigned i = blockIdx.x * WG + threadIdx.x;
    int r = -1, x = 0, y = 0, z = 0, v = 0;
    if (i < dhw) {
        const int id = ids[i];
        if (id >= 1 && id <= a.m) {
            r = id - 1;
            coords(i, (unsigned)a.H * (unsigned)a.W, a.W, x, y, z);
            v = inten[i];
        }
    }
    if (!__ballot(r >= 0)) return;                              // (wave-uniform)
    u64 s = 0;
    unsigned n = 0;
    if (r >= 0) {
        for (int k = 0; k < n_rows; ++k) {
            const int4 row = rows[k];                           // (the same address in every lane)
            const int yy = y + row.x, zz = z + row.y;
            if ((unsigned)yy < (unsigned)a.H && (unsigned)zz < (unsigned)a.D) {
                const int lo = max(x - row.z, 0), hi = min(x + row.z, a.W - 1);
                const uint32_t *const p = prefix + ((size_t)zz * a.H + yy) * (size_t)(a.W + 1);
                s += p[hi + 1] - p[lo];
                n += (unsigned)(hi - lo + 1);
            }
        }
    }
    peel<64>(r, -1, [&](int r0, bool mine, u64 mm, int leader) {
        const int slot = wave_take(cursor + r0, mm, leader);
        if (mine) {
            const int4 sg = seg[r0];
            if (slot < sg.y) {
                VspCand c;
                c.sn = (s << 24) | n;                           // (n <= 2^23, s < 2^39)
                c.index = (int)i;
                c.tag = (r0 << 1) | (v == table[r0].imax);
                cand[(size_t)sg.x + slot] = c;
            }
        }
    });
}

// ---- peaks: the best candidate of a segment, a workgroup per component ----------------------------------------------------------------------
// (sn, index) a is better than b when its mean is larger, s_a n_b > s_b n_a in 64 unsigned bits, or the means are equal and its index is
// smaller: a total order on the candidates of a component, so the maximum does not depend on the order in which they are met.  The
// empty state (s = 0, n = 1, index NONE) loses against every candidate.
struct Best { u64 sn; int index; };
__device__ __forceinline__ Best better(Best a, Best b)
{
    const u64 l = (a.sn >> 24) * (b.sn & 0xFFFFFFull), r = (b.sn >> 24) * (a.sn & 0xFFFFFFull);
    return l > r || (l == r && a.index < b.index) ? a : b;
}
__device__ __forceinline__ Best wave_best(Best v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        Best w;
        w.sn = __shfl_xor(v.sn, o, 64);
        w.index = __shfl_xor(v.index, o, 64);
        v = better(v, w);
    }
    return v;
}

__global__ __launch_bounds__(256) void k_vsp_peaks(const VspCand *__restrict__ cand, const int4 *__restrict__ seg, long long *__restrict__ peaks)
{
    __shared__ Best s_w[2][4];
    const int r = blockIdx.x;
    const int4 sg = seg[r];
    if (sg.y <= 0) return;                                      // (uniform) no voxel: the entry stays all-zero
    const VspCand *const C = cand + sg.x;
    Best g{ 1ull, NONE }, l{ 1ull, NONE };
    for (int k = threadIdx.x; k < sg.y; k += WG) {
        const VspCand c = C[k];
        const Best b{ c.sn, c.index };
        g = better(g, b);
        if (c.tag & 1) l = better(l, b);
    }
    g = wave_best(g);
    l = wave_best(l);
    if ((threadIdx.x & 63) == 0) {
        s_w[0][threadIdx.x >> 6] = g;
        s_w[1][threadIdx.x >> 6] = l;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int which = 0; which < 2; ++which) {
            Best b = s_w[which][0];
            for (int w = 1; w < 4; ++w) b = better(b, s_w[which][w]);
            peaks[6 * r + 3 * which + 0] = (long long)(b.sn >> 24);
            peaks[6 * r + 3 * which + 1] = (long long)(b.sn & 0xFFFFFFull);
            peaks[6 * r + 3 * which + 2] = b.index;
        }
    }
}

// ---- rank: how many candidates of the segment have a smaller index ---------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_vsp_rank(const VspCand *__restrict__ cand, const int4 *__restrict__ seg,
                                                  const VspItem *__restrict__ items, int *rank)
{
    __shared__ int s_b[VSP_TILE];
    const VspItem it = items[blockIdx.x];
    const int4 sg = seg[it.comp];
    const VspCand *const C = cand + sg.x;
    const int n = sg.y;
    const int ai = it.a_tile * VSP_TILE + (int)threadIdx.x;
    const bool valid = ai < n;
    const int mine = C[valid ? ai : 0].index;                   // (an item's segment holds at least one candidate)
    int below = 0;
    for (int t = 0; t < it.b_tiles; ++t) {
        const int b0 = (it.b_first + t) * VSP_TILE;
        const int nb = min(VSP_TILE, n - b0);
        if (nb <= 0) break;                                     // (uniform over the workgroup)
        __syncthreads();
        if ((int)threadIdx.x < nb) s_b[threadIdx.x] = C[b0 + threadIdx.x].index;
        __syncthreads();
#pragma unroll 8
        for (int j = 0; j < nb; ++j) below += s_b[j] < mine;    // (the same address in every lane: a broadcast)
    }
    if (valid && below) atomicAdd(rank + (size_t)sg.x + ai, below);
}

// ---- place: candidate -> the point at its rank ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_vsp_place(const VspCand *__restrict__ cand, const int *__restrict__ rank,
                                                   const uint16_t *__restrict__ inten, VolumeSpatialArgs a, const int4 *__restrict__ seg,
                                                   size_t candidates, int4 *__restrict__ points)
{
    const size_t k = (size_t)blockIdx.x * WG + threadIdx.x;
    if (k >= candidates) return;
    const VspCand c = cand[k];
    const int4 sg = seg[c.tag >> 1];
    if (sg.z < 0) return;                                       // not searched
    const int at = rank[k];
    if (at >= sg.y) return;                                     // (cannot occur: the indices of a segment are distinct)
    int x, y, z;
    coords((unsigned)c.index, (unsigned)a.H * (unsigned)a.W, a.W, x, y, z);
    points[(size_t)sg.z + at] = make_int4(x * a.ux, y * a.uy, z * a.uz, (int)inten[c.index] - sg.w);
}

// ---- pairs: the hot path -------------------------------------------------------------------------------------------------------------------
// 1 / sqrt(d2) for an integer 1 <= d2 < 2^31: the single-precision estimate (1 ulp of a float on (float)d2: relative error below 2^-22),
// then two Newton steps y <- y + (y / 2)(1 - x y^2) in double.  A step takes a relative error e to 3/2 e^2: 9e-14 after the first,
// 1e-26 after the second.  The roundings of the last step are those of x * y (it moves 1 - x y^2 by at most 2^-53, and so y by half
// of that relative to y) and of the final fused multiply-add (2^-53): the result is within 0.75 ulp, far inside the 4 ulp of the contract.
__device__ __forceinline__ double inv_sqrt(int d2)
{
    const double x = (double)d2;
    double y = (double)__builtin_amdgcn_rsqf((float)d2);
    double e = __builtin_fma(-(x * y), y, 1.0);
    y = __builtin_fma(0.5 * y, e, y);
    e = __builtin_fma(-(x * y), y, 1.0);
    y = __builtin_fma(0.5 * y, e, y);
    return y;
}

// A lane holds point ai of the a-tile and meets the points of the item's b-tiles in ascending order; in the diagonal tile it takes j > i
// only.  The integer factors y_i + y_j, y_i y_j, (y_i - y_j)^2 are below 2^34: formed in double from exact conversions they are the exact
// integers.  The lane's four sums are added across the wave by the butterfly (the same tree on every run), the four waves' in the order
// 0, 1, 2, 3 -> slots[item].
__global__ __launch_bounds__(256) void k_vsp_pairs(const int4 *__restrict__ points, const int4 *__restrict__ seg,
                                                   const VspItem *__restrict__ items, double *__restrict__ slots)
{
    __shared__ int4 s_b[VSP_TILE];
    __shared__ double s_w[4][4];
    const VspItem it = items[blockIdx.x];
    const int4 sg = seg[it.comp];
    const int4 *const P = points + sg.z;
    const int n = sg.y;
    const int ai = it.a_tile * VSP_TILE + (int)threadIdx.x;
    const bool valid = ai < n;
    const int4 a = P[valid ? ai : 0];                           // (an item's segment holds at least two points)
    const double ya = (double)a.w;
    double s0 = 0.0, s1 = 0.0, s2 = 0.0, s3 = 0.0;
    for (int t = 0; t < it.b_tiles; ++t) {
        const int b0 = (it.b_first + t) * VSP_TILE;
        const int nb = min(VSP_TILE, n - b0);
        if (nb <= 0) break;                                     // (uniform over the workgroup)
        __syncthreads();
        if ((int)threadIdx.x < nb) s_b[threadIdx.x] = P[b0 + threadIdx.x];
        __syncthreads();
        const int after = !valid ? VSP_TILE : it.b_first + t == it.a_tile ? (int)threadIdx.x : -1;     // the lane takes the j above this
#pragma unroll 4
        for (int j = 0; j < nb; ++j) {
            const int4 b = s_b[j];                              // (the same address in every lane: a broadcast)
            const int dx = a.x - b.x, dy = a.y - b.y, dz = a.z - b.z;
            // (a scaled coordinate is at most 46340 by the d2 limit, so the 24-bit multiply, which runs at the full rate, is exact)
            const int d2 = __mul24(dx, dx) + __mul24(dy, dy) + __mul24(dz, dz);
            const bool take = j > after;
            const double w = take ? inv_sqrt(take ? d2 : 1) : 0.0;
            const double yb = (double)b.w, d = ya - yb;
            s0 += w;
            s1 = __builtin_fma(w, ya + yb, s1);
            s2 = __builtin_fma(w, ya * yb, s2);
            s3 = __builtin_fma(w, d * d, s3);
        }
    }
    s0 = wave_sum(s0); s1 = wave_sum(s1); s2 = wave_sum(s2); s3 = wave_sum(s3);
    if ((threadIdx.x & 63) == 0) {
        double *const w = s_w[threadIdx.x >> 6];
        w[0] = s0; w[1] = s1; w[2] = s2; w[3] = s3;
    }
    __syncthreads();
    if (threadIdx.x < 4) {
        const int f = threadIdx.x;
        slots[4 * (size_t)blockIdx.x + f] = ((s_w[0][f] + s_w[1][f]) + s_w[2][f]) + s_w[3][f];
    }
}

bool fits(const VolumeSpatialArgs &a)
{
    if (a.D < 1 || a.H < 1 || a.W < 1 || a.m < 1 || a.ux < 1 || a.uy < 1 || a.uz < 1) return false;
    return (long long)a.D * a.H * a.W < (1LL << 31);
}

inline unsigned blocks(size_t n) { return (unsigned)((n + WG - 1) / WG); }

}  // namespace vsp

hipError_t launch_volume_spatial_sums(const int32_t *ids, const uint16_t *intensity, const VolumeSpatialArgs &a, ::mi_unet_vspatial *table,
                                      hipStream_t s)
{
    if (!ids || !intensity || !table || !vsp::fits(a)) return hipErrorInvalidValue;
    const unsigned dhw = (unsigned)a.D * (unsigned)a.H * (unsigned)a.W;
    if (hipError_t e = hipMemsetAsync(table, 0, (size_t)a.m * sizeof(::mi_unet_vspatial), s)) return e;
    const unsigned waves = (dhw + 64u * vsp::RUN - 1) / (64u * vsp::RUN);
    hipLaunchKernelGGL(vsp::k_vsp_sums, dim3((waves + 3) / 4), dim3(vsp::WG), 0, s, ids, intensity, a.H, a.W, dhw, a.m, table);
    return hipGetLastError();
}

hipError_t launch_volume_spatial_prefix(const uint16_t *intensity, const VolumeSpatialArgs &a, uint32_t *prefix, hipStream_t s)
{
    if (!intensity || !prefix || !vsp::fits(a)) return hipErrorInvalidValue;
    const unsigned rows = (unsigned)a.D * (unsigned)a.H;
    hipLaunchKernelGGL(vsp::k_vsp_prefix, dim3((rows + 3) / 4), dim3(vsp::WG), 0, s, intensity, a.W, rows, prefix);
    return hipGetLastError();
}

hipError_t launch_volume_spatial_fill(const int32_t *ids, const uint16_t *intensity, const uint32_t *prefix, const VolumeSpatialArgs &a,
                                      const ::mi_unet_vspatial *table, const int4 *seg, const int4 *rows, int n_rows, int *cursor, int *rank,
                                      size_t candidates, VspCand *cand, hipStream_t s)
{
    if (!ids || !intensity || !prefix || !table || !seg || !rows || n_rows < 1 || !cursor || !rank || !cand || !vsp::fits(a))
        return hipErrorInvalidValue;
    const unsigned dhw = (unsigned)a.D * (unsigned)a.H * (unsigned)a.W;
    if (hipError_t e = hipMemsetAsync(cursor, 0, (size_t)a.m * sizeof(int), s)) return e;
    if (hipError_t e = hipMemsetAsync(rank, 0, candidates * sizeof(int), s)) return e;
    hipLaunchKernelGGL(vsp::k_vsp_fill, dim3(vsp::blocks(dhw)), dim3(vsp::WG), 0, s, ids, intensity, prefix, a, dhw, table, seg, rows, n_rows,
                       cursor, cand);
    return hipGetLastError();
}

hipError_t launch_volume_spatial_peaks(const VspCand *cand, const int4 *seg, int m, long long *peaks, hipStream_t s)
{
    if (!cand || !seg || !peaks || m < 1) return hipErrorInvalidValue;
    if (hipError_t e = hipMemsetAsync(peaks, 0, (size_t)m * 6 * sizeof(long long), s)) return e;
    hipLaunchKernelGGL(vsp::k_vsp_peaks, dim3((unsigned)m), dim3(vsp::WG), 0, s, cand, seg, peaks);
    return hipGetLastError();
}

hipError_t launch_volume_spatial_rank(const VspCand *cand, const int4 *seg, const VspItem *items, int n_items, int *rank, hipStream_t s)
{
    if (!cand || !seg || !items || !rank || n_items < 1) return hipErrorInvalidValue;
    hipLaunchKernelGGL(vsp::k_vsp_rank, dim3((unsigned)n_items), dim3(vsp::WG), 0, s, cand, seg, items, rank);
    return hipGetLastError();
}

hipError_t launch_volume_spatial_place(const VspCand *cand, const int *rank, const uint16_t *intensity, const VolumeSpatialArgs &a,
                                       const int4 *seg, size_t candidates, int4 *points, hipStream_t s)
{
    if (!cand || !rank || !intensity || !seg || !points || candidates < 1 || !vsp::fits(a)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(vsp::k_vsp_place, dim3(vsp::blocks(candidates)), dim3(vsp::WG), 0, s, cand, rank, intensity, a, seg, candidates, points);
    return hipGetLastError();
}

hipError_t launch_volume_spatial_pairs(const int4 *points, const int4 *seg, const VspItem *items, int n_items, double *slots, hipStream_t s)
{
    if (!points || !seg || !items || !slots || n_items < 1) return hipErrorInvalidValue;
    hipLaunchKernelGGL(vsp::k_vsp_pairs, dim3((unsigned)n_items), dim3(vsp::WG), 0, s, points, seg, items, slots);
    return hipGetLastError();
}

}  // namespace miunet
