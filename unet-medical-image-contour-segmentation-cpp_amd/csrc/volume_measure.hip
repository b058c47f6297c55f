// volume_measure.hip -- per component of a labelled stack its sums, its run ends and its longest diameters (include/mi_unet.h:
// mi_unet_volume_measure).  k_vms_sums: a lane per voxel, the wave reduces per distinct id and carries an id's sums until
// the id changes (wave.h's peel).  k_vms_fill: every run end of a searched component into the component's segment.  k_vms_pairs, the
// hot path: an N-body tiling over the upper-triangular tile pairs of a segment, a point per lane against a tile in LDS.  k_vms_ends: the
// smallest partner of the winning (d2, p).  Every result is an integer sum, minimum or maximum, so nothing depends on the order in which
// atomics arrive or in which a segment was filled; no workgroup waits for another.  gfx950 only.
#include "../../include/mi_unet.h"
#include "kernel_common.h"
#include "kernels.h"
#include "wave.h"

namespace miunet {

namespace vms {

using namespace wave;

constexpr unsigned WG = 256;                // lanes per workgroup; = VMS_TILE in k_vms_pairs
constexpr int RUN = 16;                     // 64-voxel segments a wave of k_vms_sums carries an id over
constexpr int GROUPS = 4;                   // distinct ids of a segment that are reduced across the wave; lanes beyond them add their own
constexpr int NONE = 0x7FFFFFFF;
static_assert(VMS_TILE == (int)WG, "a lane per point of the a-tile, a lane per point of the b-tile's load");

// the sums of one id: n voxels, e run ends, the nine coordinate sums (x, y, z, xx, yy, zz, xy, xz, yz), si, sii, lo / hi of the intensity
struct Acc {
    int n, e, lo, hi;
    long long s[11];
};

// field f of the entry, 0 .. 14: voxels, ends, imin, imax, the nine coordinate sums, si, sii.  One atomic; a wave that holds the same acc in
// every lane issues fifteen of them from fifteen lanes at once.  The sum is picked by selects: a run-time index would put acc into scratch.
__device__ __forceinline__ void add_field(mi_unet_vmeasure *c, const Acc &a, int f)
{
    if (f == 0) atomicAdd(&c->voxels, a.n);
    else if (f == 1) atomicAdd(&c->ends, a.e);
    else if (f == 2) atomicMax(&c->imin, 65535 - a.lo);         // (turned round by the caller: 0 = no voxel yet)
    else if (f == 3) atomicMax(&c->imax, a.hi);
    else {
        long long v = 0;
#pragma unroll
        for (int j = 0; j < 11; ++j) v = f - 4 == j ? a.s[j] : v;
        atomicAdd(reinterpret_cast<u64 *>(&c->sx) + (f - 4), (u64)v);
    }
}

// ---- sums: one lane per voxel, consecutive lanes along x -------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_vms_sums(const int32_t *__restrict__ ids, const uint16_t *__restrict__ inten, int H, int W,
                                                  unsigned dhw, int m, mi_unet_vmeasure *table)
{
    const int lane = threadIdx.x & 63;
    const long long first = (((long long)blockIdx.x * WG + threadIdx.x) >> 6) * (64LL * RUN);
    const unsigned hw = (unsigned)H * (unsigned)W;
    int ar = -1;                                                // (wave-uniform) the id carried, and its sums
    Acc acc;
    auto reset = [&]() {
        acc.n = 0; acc.e = 0; acc.lo = 65535; acc.hi = 0;
#pragma unroll
        for (int j = 0; j < 11; ++j) acc.s[j] = 0;
    };
    auto flush = [&]() {
        if (ar >= 0 && lane < 15) add_field(table + ar, acc, lane);
    };
    reset();
    for (int sg = 0; sg < RUN; ++sg) {
        if (first + 64LL * sg >= (long long)dhw) break;         // (wave-uniform)
        const long long i = first + 64LL * sg + lane;
        int r = -1, e = 0, v = 0, x = 0, y = 0, z = 0;
        if (i < (long long)dhw) {
            const int id = ids[i];
            if (id >= 1 && id <= m) {
                r = id - 1;
                z = (int)((unsigned)i / hw);
                const int rem = (int)((unsigned)i - (unsigned)z * hw);
                y = rem / W;
                x = rem - y * W;
                e = (x == 0 || ids[i - 1] != id) || (x == W - 1 || ids[i + 1] != id);
                if (inten) v = inten[i];
            }
        }
        peel<GROUPS>(r, -1, [&](int r0, bool mine, u64 mm, int) {
            if (r0 != ar) {
                flush();
                reset();
                ar = r0;
            }
            acc.n += __popcll(mm);
            acc.e += __popcll(__ballot(mine && e));
            const long long cx = mine ? x : 0, cy = mine ? y : 0, cz = mine ? z : 0, cv = mine ? v : 0;
            acc.s[0] += wave_sum(cx); acc.s[1] += wave_sum(cy); acc.s[2] += wave_sum(cz);
            acc.s[3] += wave_sum(cx * cx); acc.s[4] += wave_sum(cy * cy); acc.s[5] += wave_sum(cz * cz);
            acc.s[6] += wave_sum(cx * cy); acc.s[7] += wave_sum(cx * cz); acc.s[8] += wave_sum(cy * cz);
            if (inten) {                                        // (uniform)
                acc.s[9] += wave_sum(cv); acc.s[10] += wave_sum(cv * cv);
                acc.lo = min(acc.lo, wave_min(mine ? v : 65535));
                acc.hi = max(acc.hi, wave_max(mine ? v : 0));
            }
        });
        if (r >= 0) {                                           // a segment of many small components: the lane adds its own voxel
            Acc one;
            one.n = 1; one.e = e; one.lo = v; one.hi = v;
            const long long cx = x, cy = y, cz = z, cv = v;
            one.s[0] = cx; one.s[1] = cy; one.s[2] = cz; one.s[3] = cx * cx; one.s[4] = cy * cy; one.s[5] = cz * cz;
            one.s[6] = cx * cy; one.s[7] = cx * cz; one.s[8] = cy * cz; one.s[9] = cv; one.s[10] = cv * cv;
            for (int f = 0; f < (inten ? 15 : 13); ++f)
                if (inten || (f != 2 && f != 3)) add_field(table + r, one, f);
        }
    }
    flush();
}

// ---- fill: every run end of a searched component into the component's segment ----------------------------------------------------------------
// A wave takes one slot range per distinct id among its run ends (one atomic each); the order inside a segment is that of arrival, which
// no result depends on.  A slot at or past the segment's size cannot occur while `ends` is exact; it is dropped all the same.
__global__ __launch_bounds__(256) void k_vms_fill(const int32_t *__restrict__ ids, VolumeMeasureArgs a, unsigned dhw,
                                                  const int2 *__restrict__ seg, int *cursor, int4 *__restrict__ points)
{
    const unsigned i = blockIdx.x * WG + threadIdx.x;
    int r = -1, x = 0, y = 0, z = 0;
    if (i < dhw) {
        const int id = ids[i];
        if (id >= 1 && id <= a.m && seg[id - 1].y > 0) {
            const unsigned hw = (unsigned)a.H * (unsigned)a.W;
            z = (int)(i / hw);
            const int rem = (int)(i - (unsigned)z * hw);
            y = rem / a.W;
            x = rem - y * a.W;
            if ((x == 0 || ids[i - 1] != id) || (x == a.W - 1 || ids[i + 1] != id)) r = id - 1;
        }
    }
    peel<64>(r, -1, [&](int r0, bool mine, u64 mm, int leader) {
        const int slot = wave_take(cursor + r0, mm, leader);
        if (mine) {
            const int2 sg = seg[r0];
            if (slot < sg.y) points[(size_t)sg.x + slot] = make_int4(x * a.ux, y * a.uy, z * a.uz, (int)i);
        }
    });
}

// ---- pairs: the hot path -------------------------------------------------------------------------------------------------------------------
// A lane's state is its best pair over all partners and over the partners with equal z, each as one 64-bit key (d2 << 32) | ~index of
// the partner: the larger d2 wins, among equal d2 the smaller partner index, so the state does not depend on the order of the partners and
// a pair costs one 64-bit compare and two selects.  The tile in LDS holds ~index.  The lane's best pair is then (min, max) of its own
// index and the partner's: were a partner below the lane's own index, that partner is the pair's p.  The workgroup raises the component's
// key to (d2 << 31) | (2^31 - 1 - p): d2 descending, then p ascending.
__global__ __launch_bounds__(256) void k_vms_pairs(const int4 *__restrict__ points, const int2 *__restrict__ seg,
                                                   const VmsItem *__restrict__ items, u64 *keys)
{
    __shared__ int4 s_b[VMS_TILE];
    const VmsItem it = items[blockIdx.x];
    const int2 sg = seg[it.comp];
    const int4 *const P = points + sg.x;
    const int n = sg.y;
    const int ai = it.a_tile * VMS_TILE + (int)threadIdx.x;
    const bool valid = ai < n;
    const int4 a = P[valid ? ai : 0];                           // (an item's segment holds at least one point)
    u64 best = 0, best_a = 0;                                   // (every key of a pair is above 0: an index is below 2^31)
    for (int t = 0; t < it.b_tiles; ++t) {
        const int b0 = (it.b_first + t) * VMS_TILE;
        const int nb = min(VMS_TILE, n - b0);
        if (nb <= 0) break;                                     // (uniform over the workgroup)
        __syncthreads();
        if ((int)threadIdx.x < nb) {
            const int4 b = P[b0 + threadIdx.x];
            s_b[threadIdx.x] = make_int4(b.x, b.y, b.z, ~b.w);
        }
        __syncthreads();
#pragma unroll 4
        for (int j = 0; j < nb; ++j) {
            const int4 b = s_b[j];                              // (the same address in every lane: a broadcast)
            const int dx = a.x - b.x, dy = a.y - b.y, dz = a.z - b.z;
            // (a scaled coordinate is at most 46340 by the d2 limit, so the 24-bit multiply, which runs at the full rate, is exact)
            const u64 key = ((u64)(unsigned)(__mul24(dx, dx) + __mul24(dy, dy) + __mul24(dz, dz)) << 32) | (unsigned)b.w;
            best = key > best ? key : best;
            best_a = dz == 0 && key > best_a ? key : best_a;
        }
    }
    u64 k = 0, k_a = 0;
    if (valid && best) k = ((best >> 32) << 31) | (u64)(unsigned)(NONE - min(a.w, (int)~(unsigned)best));
    if (valid && best_a) k_a = ((best_a >> 32) << 31) | (u64)(unsigned)(NONE - min(a.w, (int)~(unsigned)best_a));
    k = wave_max(k);
    k_a = wave_max(k_a);
    if ((threadIdx.x & 63) == 0) {
        if (k) atomicMax(keys + 2 * it.comp, k);
        if (k_a) atomicMax(keys + 2 * it.comp + 1, k_a);
    }
}

// ---- ends: the smallest partner of the winning (d2, p), a workgroup per component -------------------------------------------------------------
// Every partner of p at d2 has an index >= p: a smaller one would have been the pair's p.
__global__ __launch_bounds__(256) void k_vms_ends(const int4 *__restrict__ points, const int2 *__restrict__ seg, const u64 *__restrict__ keys,
                                                  VolumeMeasureArgs a, int32_t *__restrict__ diam)
{
    __shared__ int s_w[4];
    const int r = blockIdx.x;
    const int2 sg = seg[r];
    if (sg.y <= 0) return;                                      // (uniform) not searched: the caller writes its fields
    const int4 *const P = points + sg.x;
    for (int which = 0; which < 2; ++which) {
        const u64 key = keys[2 * r + which];
        const int d2 = (int)(key >> 31), p = NONE - (int)(key & 0x7FFFFFFFull);
        const unsigned hw = (unsigned)a.H * (unsigned)a.W;
        const int z = (int)((unsigned)p / hw), rem = (int)((unsigned)p - (unsigned)z * hw), y = rem / a.W, x = rem - y * a.W;
        const int px = x * a.ux, py = y * a.uy, pz = z * a.uz;
        int q = NONE;
        for (int i = threadIdx.x; i < sg.y; i += WG) {
            const int4 b = P[i];
            const int dx = px - b.x, dy = py - b.y, dz = pz - b.z;
            if (dx * dx + dy * dy + dz * dz == d2 && (which == 0 || dz == 0)) q = min(q, b.w);
        }
        q = wave_min(q);
        __syncthreads();
        if ((threadIdx.x & 63) == 0) s_w[threadIdx.x >> 6] = q;
        __syncthreads();
        if (threadIdx.x == 0) {
            q = min(min(s_w[0], s_w[1]), min(s_w[2], s_w[3]));
            const bool ok = key != 0 && q != NONE;              // (always, for a segment that holds the component's run ends)
            diam[6 * r + 3 * which + 0] = ok ? d2 : -1;
            diam[6 * r + 3 * which + 1] = ok ? p : -1;
            diam[6 * r + 3 * which + 2] = ok ? q : -1;
        }
    }
}

bool fits(const VolumeMeasureArgs &a)
{
    if (a.D < 1 || a.H < 1 || a.W < 1 || a.m < 1 || a.ux < 1 || a.uy < 1 || a.uz < 1) return false;
    return (long long)a.D * a.H * a.W < (1LL << 31);
}

inline unsigned blocks(unsigned n) { return (n + WG - 1) / WG; }

}  // namespace vms

hipError_t launch_volume_measure_sums(const int32_t *ids, const uint16_t *intensity, const VolumeMeasureArgs &a, ::mi_unet_vmeasure *table,
                                      hipStream_t s)
{
    if (!ids || !table || !vms::fits(a)) return hipErrorInvalidValue;
    const unsigned dhw = (unsigned)a.D * (unsigned)a.H * (unsigned)a.W;
    if (hipError_t e = hipMemsetAsync(table, 0, (size_t)a.m * sizeof(::mi_unet_vmeasure), s)) return e;
    const unsigned waves = (dhw + 64u * vms::RUN - 1) / (64u * vms::RUN);
    hipLaunchKernelGGL(vms::k_vms_sums, dim3((waves + 3) / 4), dim3(vms::WG), 0, s, ids, intensity, a.H, a.W, dhw, a.m, table);
    return hipGetLastError();
}

hipError_t launch_volume_measure_fill(const int32_t *ids, const VolumeMeasureArgs &a, const int2 *seg, int *cursor, unsigned long long *keys,
                                      int4 *points, hipStream_t s)
{
    if (!ids || !seg || !cursor || !keys || !points || !vms::fits(a)) return hipErrorInvalidValue;
    const unsigned dhw = (unsigned)a.D * (unsigned)a.H * (unsigned)a.W;
    if (hipError_t e = hipMemsetAsync(cursor, 0, (size_t)a.m * sizeof(int), s)) return e;
    if (hipError_t e = hipMemsetAsync(keys, 0, (size_t)a.m * 2 * sizeof(unsigned long long), s)) return e;
    hipLaunchKernelGGL(vms::k_vms_fill, dim3(vms::blocks(dhw)), dim3(vms::WG), 0, s, ids, a, dhw, seg, cursor, points);
    return hipGetLastError();
}

hipError_t launch_volume_measure_pairs(const int4 *points, const int2 *seg, const VmsItem *items, int n_items, unsigned long long *keys,
                                       hipStream_t s)
{
    if (!points || !seg || !items || !keys || n_items < 1) return hipErrorInvalidValue;
    hipLaunchKernelGGL(vms::k_vms_pairs, dim3((unsigned)n_items), dim3(vms::WG), 0, s, points, seg, items, keys);
    return hipGetLastError();
}

hipError_t launch_volume_measure_ends(const int4 *points, const int2 *seg, const unsigned long long *keys, const VolumeMeasureArgs &a,
                                      int32_t *diam, hipStream_t s)
{
    if (!points || !seg || !keys || !diam || !vms::fits(a)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(vms::k_vms_ends, dim3((unsigned)a.m), dim3(vms::WG), 0, s, points, seg, keys, a, diam);
    return hipGetLastError();
}

}  // namespace miunet
