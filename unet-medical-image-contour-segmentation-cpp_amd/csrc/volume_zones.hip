// volume_zones.hip -- per component of a labelled stack its grey-level run-length and size-zone matrices (include/mi_unet.h:
// mi_unet_volume_zones), on the key stack that volume_texture.hip's launch_volume_texture_keys makes.  k_vzn_voxels: a
// lane per voxel, a wave carries a component's count until the component changes (wave.h's peel).  k_vzn_runs, the hot path: a
// tile of keys with the halo of the backward neighbours in LDS; the lane whose backward neighbour has another key walks its run forward,
// and the lanes of a wave that name one cell merge before the atomic.  k_vzn_init / k_vzn_merge: 7.9's lock-free union-find on keys.
// k_vzn_sizes: a wave carries a root's count.  k_vzn_flags / k_vzn_scan / k_vzn_list: the roots in raster order at scanned positions;
// k_vzn_tally: the zones of every component and its largest.
// k_vzn_finish: the 13-offset table from its two parts, and the table entries.  Every result is an integer sum, minimum or maximum, so
// nothing depends on the order in which atomics arrive; no workgroup waits for another; every walk ends at the volume's border.
// gfx950 only.
#include "../../include/mi_unet.h"
#include "cc_common.h"
#include "kernel_common.h"
#include "kernels.h"
#include "key_tile.h"
#include "wave.h"

namespace miunet {

namespace vzn {

using namespace wave;
using namespace key_tile;

constexpr unsigned WG = 256;                // lanes per workgroup
constexpr int RUN = 16;                     // 64-voxel segments a wave of k_vzn_voxels / k_vzn_sizes carries a count over
constexpr int GROUPS = 4;                   // distinct owners of a segment that are reduced across the wave; lanes beyond them add their own
constexpr int MERGE = 3;                    // distinct cells of one offset that a wave merges; lanes beyond them add their own
constexpr int KZ = TZ + 1;                  // key_tile.h's tile with the slice before it: z - 1 .. z
constexpr int TILE_KEYS = KX * KY * KZ;
constexpr int SCAN = 1024;                  // counts a workgroup of k_vzn_scan takes, four a lane
// ---- keys of more components than launch_volume_texture_keys takes at once (m L^2 above 2^22 while m L R is not) -----------------------------
// part: the ids of components first .. first + count - 1, renumbered from 1, every other voxel 0: what the launcher turns into keys.
__global__ __launch_bounds__(256) void k_vzn_part(const int32_t *__restrict__ ids, unsigned dhw, int first, int count, int32_t *__restrict__ part)
{
    const unsigned i = blockIdx.x * WG + threadIdx.x;
    if (i >= dhw) return;
    const int id = ids[i];
    part[i] = id > first && id <= first + count ? id - first : 0;
}
// join: the part's keys, their component numbers moved back by `first`, into the key stack (zeroed by the caller; the parts are disjoint)
__global__ __launch_bounds__(256) void k_vzn_join(const int32_t *__restrict__ part, unsigned dhw, int first, int32_t *__restrict__ keys)
{
    const unsigned i = blockIdx.x * WG + threadIdx.x;
    if (i >= dhw) return;
    const int k = part[i];
    if (k) keys[i] = k + (first << 8);
}

// ---- voxels per component; one lane per voxel ------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_vzn_voxels(const int32_t *__restrict__ keys, unsigned dhw, VznAcc *acc)
{
    const int lane = threadIdx.x & 63;
    const long long first = (((long long)blockIdx.x * WG + threadIdx.x) >> 6) * (64LL * RUN);
    int ar = 0, cnt = 0;                                        // (wave-uniform) the component number carried (0: none) and its count
    auto flush = [&]() {
        if (ar && lane == 0) atomicAdd(&acc[ar - 1].voxels, cnt);
    };
    for (int sg = 0; sg < RUN; ++sg) {
        if (first + 64LL * sg >= (long long)dhw) break;         // (wave-uniform)
        const long long i = first + 64LL * sg + lane;
        int r = i < (long long)dhw ? keys[i] >> 8 : 0;
        peel<GROUPS>(r, 0, [&](int r0, bool, u64 mm, int) {
            if (r0 != ar) {
                flush();
                ar = r0; cnt = 0;
            }
            cnt += __popcll(mm);
        });
        if (r) atomicAdd(&acc[r - 1].voxels, 1);                // a segment of many small components: the lane adds its own voxel
    }
    flush();
}

// ---- runs: the hot path -----------------------------------------------------------------------------------------------------------------
// Every count goes through wave.h's merged_add.
// LDS: the keys of the tile with its halo; a position outside the volume holds 0, which ends every run.  A workgroup takes
// VTX_TILES_PER_WG tiles that follow each other along x.  A run belongs to the tile of its first voxel, so every run is counted once.
__global__ __launch_bounds__(256) void k_vzn_runs(const int32_t *__restrict__ keys, VolumeZonesArgs a, int want, int tiles_x, int tiles_y,
                                                  int n_tiles, VznAcc *acc, uint32_t *inter, uint32_t *axial)
{
    __shared__ int s_keys[TILE_KEYS];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const bool do_axial = want & VZN_WANT_AXIAL, do_inter = want & VZN_WANT_INTER;
    const int L = a.L, R = a.R;
    const int t_end = min(n_tiles, ((int)blockIdx.x + 1) * VTX_TILES_PER_WG);
    for (int t = (int)blockIdx.x * VTX_TILES_PER_WG; t < t_end; ++t) {
        const int3 o = tile_origin<1>(t, tiles_x, tiles_y);
        const int x0 = o.x, y0 = o.y, z0 = o.z;
        __syncthreads();                                        // the tile before is done with s_keys
        load_key_tile<KZ, 1>(s_keys, keys, o, a.D, a.H, a.W);
        __syncthreads();
#pragma unroll 1
        for (int it = 0; it < ROWS / 4; ++it) {
            const int row = wave * (ROWS / 4) + it;
            const int lz = row / TY + 1, ly = row % TY + 1, lx = lane + 1;
            const int *const p = s_keys + lz * (KX * KY) + ly * KX + lx;
            const int k = *p;
            if (!__ballot(k != 0)) continue;                    // (wave-uniform) a row of no component
            const int id = k >> 8;
            const unsigned row_cell = ((unsigned)(id - 1) * (unsigned)L + (unsigned)(k & 255)) * (unsigned)R;    // (below 2^22; only read when k != 0)
            int best = 0;                                       // the longest run this voxel starts
            auto offset = [&](int dx, int dy, int dz, uint32_t *tab, bool inter_half) {
                const int step = dz * (KX * KY) + dy * KX + dx;
                const bool start = k != 0 && p[-step] != k;     // (the backward neighbour lies in the halo; outside the volume it is 0)
                int n = 0;
                if (start) {
                    n = 1;
                    int qx = lx + dx, qy = ly + dy, qz = lz + dz;
                    const int *q = p + step;
                    bool in_box;
                    for (;;) {                                  // inside the tile and its halo: LDS
                        in_box = qx >= 0 && qx < KX && qy >= 0 && qy < KY && qz < KZ;
                        if (!in_box || *q != k) break;
                        ++n; qx += dx; qy += dy; qz += dz; q += step;
                    }
                    if (!in_box) {                              // beyond it: memory, until the key changes or the volume ends
                        int X = x0 + qx, Y = y0 + qy, Z = z0 + qz;
                        while (X >= 0 && X < a.W && Y >= 0 && Y < a.H && Z < a.D && keys[((size_t)Z * a.H + Y) * a.W + X] == k) {
                            ++n; X += dx; Y += dy; Z += dz;
                        }
                    }
                    if (n > R) atomicAdd(inter_half ? &acc[id - 1].clamped_inter : &acc[id - 1].clamped_axial, 1ULL);
                    best = max(best, n);
                }
                merged_add<MERGE>(tab, start, row_cell + (unsigned)(min(n, R) - 1));
            };
            if (do_axial) {
                offset(1, 0, 0, axial, false);
                offset(-1, 1, 0, axial, false);
                offset(0, 1, 0, axial, false);
                offset(1, 1, 0, axial, false);
            }
            if (do_inter) {
#pragma unroll
                for (int dy = -1; dy <= 1; ++dy)
#pragma unroll
                    for (int dx = -1; dx <= 1; ++dx) offset(dx, dy, 1, inter, true);
                // the longest run: one atomic per wave and component for the first two components of the row, and only when a plain
                // read does not already show it
                int rid = best > 0 ? id : 0;
                peel<2>(rid, 0, [&](int r0, bool mine, u64, int leader) {
                    const int v = wave_max(mine ? best : 0);
                    if (lane == leader) raise(&acc[r0 - 1].longest, v);
                });
                if (rid) raise(&acc[rid - 1].longest, best);
            }
        }
    }
}

// ---- zones: 7.9's union-find on keys -----------------------------------------------------------------------------------------------------
// init: the parent of a voxel is the first voxel of its run of one key along x inside its 64-lane segment; a run ends at x = W - 1.
__global__ __launch_bounds__(256) void k_vzn_init(const int32_t *__restrict__ keys, unsigned dhw, int W, int *parent)
{
    const unsigned i = blockIdx.x * WG + threadIdx.x;
    const int lane = threadIdx.x & 63;
    const int k = i < dhw ? keys[i] : 0;
    const int kl = __shfl_up(k, 1, 64);
    const bool joined = lane > 0 && k != 0 && kl == k && i % (unsigned)W != 0;
    const u64 starts = __ballot(!joined) & ((2ULL << lane) - 1ULL);                 // (lane 0 always starts one, so it is never 0)
    const int start_lane = 63 - __builtin_clzll(starts);
    if (i < dhw) parent[i] = (int)i - (lane - start_lane);
}

// merge: a voxel unites with those of its 13 earlier neighbours that carry its key, EXCEPT where the union is implied:
//   x     the left neighbour is in the voxel's run (k_vzn_init) unless the run was cut at a 64-lane boundary: lane 0 unites there;
//   shift for any other offset d: the left neighbour p - ex carries the key and so does (p + d) - ex: p - ex makes that union (or it is
//         implied in turn), and both rows are joined along x;
//   bridge for an offset with two or three non-zero components: a voxel of the key at p + a part of d joins p and p + d by two unions of
//         offsets with fewer components.
// (The order by (components of the offset, x) is well-founded, so every implied union rests on ones that are made.)  Every union is
// pp::unite; its loop ends by its own data.
__global__ __launch_bounds__(256) void k_vzn_merge(const int32_t *__restrict__ keys, VolumeZonesArgs a, unsigned dhw, int *parent)
{
    const unsigned i = blockIdx.x * WG + threadIdx.x;
    if (i >= dhw) return;
    const int k = keys[i];
    if (!k) return;
    const int W = a.W, H = a.H, D = a.D;
    const int x = (int)(i % (unsigned)W), y = (int)((i / (unsigned)W) % (unsigned)H), z = (int)(i / ((unsigned)W * (unsigned)H));
    auto same = [&](int dx, int dy, int dz) {
        const int X = x + dx, Y = y + dy, Z = z + dz;
        return X >= 0 && X < W && Y >= 0 && Y < H && Z >= 0 && Z < D && keys[(int)i + (dz * H + dy) * W + dx] == k;
    };
    const bool l = same(-1, 0, 0);
    if (l && (threadIdx.x & 63) == 0) pp::unite(parent, (int)i, (int)i - 1);
    for (int dz = -1; dz <= 0; ++dz)
        for (int dy = -1; dy <= (dz ? 1 : -1); ++dy)
            for (int dx = -1; dx <= 1; ++dx) {
                if (!same(dx, dy, dz)) continue;
                if (l && same(dx - 1, dy, dz)) continue;
                bool bridged = false;
                for (int pick = 1; pick < 7; ++pick) {          // the proper parts of d: bit 0 takes dx, bit 1 dy, bit 2 dz
                    const int ax = (pick & 1) ? dx : 0, ay = (pick & 2) ? dy : 0, az = (pick & 4) ? dz : 0;
                    if ((ax == 0 && ay == 0 && az == 0) || (ax == dx && ay == dy && az == dz)) continue;
                    bridged = bridged || same(ax, ay, az);
                }
                if (!bridged) pp::unite(parent, (int)i, (int)i + (dz * H + dy) * W + dx);
            }
}

// sizes: size[root] = the voxels of the zone; a wave carries a root's count over consecutive voxels before it issues it
__global__ __launch_bounds__(256) void k_vzn_sizes(const int32_t *__restrict__ keys, unsigned dhw, const int *parent, int *size)
{
    const int lane = threadIdx.x & 63;
    const long long first = (((long long)blockIdx.x * WG + threadIdx.x) >> 6) * (64LL * RUN);
    int ar = -1, cnt = 0;                                       // (wave-uniform) the root carried and its count
    auto flush = [&]() {
        if (ar >= 0 && lane == 0) atomicAdd(size + ar, cnt);
    };
    for (int sg = 0; sg < RUN; ++sg) {
        if (first + 64LL * sg >= (long long)dhw) break;         // (wave-uniform)
        const long long i = first + 64LL * sg + lane;
        int r = -1;
        if (i < (long long)dhw && keys[i] != 0) r = pp::find_root_ro(parent, (int)i);
        peel<GROUPS>(r, -1, [&](int r0, bool, u64 mm, int) {
            if (r0 != ar) {
                flush();
                ar = r0; cnt = 0;
            }
            cnt += __popcll(mm);
        });
        if (r >= 0) atomicAdd(size + r, 1);
    }
    flush();
}

__device__ __forceinline__ bool is_root(const int32_t *keys, const int *parent, unsigned i, unsigned dhw)
{
    return i < dhw && keys[i] != 0 && parent[i] == (int)i;
}

// flags: the roots among the 256 voxels of a workgroup
__global__ __launch_bounds__(256) void k_vzn_flags(const int32_t *__restrict__ keys, unsigned dhw, const int *__restrict__ parent, int *counts)
{
    __shared__ int s_n[4];
    const unsigned i = blockIdx.x * WG + threadIdx.x;
    const int total = wave_offsets(__popcll(__ballot(is_root(keys, parent, i, dhw))), s_n).y;
    if (threadIdx.x == 0) counts[blockIdx.x] = total;
}

// scan: the exclusive prefix of SCAN counts per workgroup in place, four a lane; the workgroup's sum into sums[workgroup] (or, for the
// one workgroup of the upper level, into *total)
__global__ __launch_bounds__(256) void k_vzn_scan(int *data, int n, int *sums, int *total)
{
    __shared__ int s_w[4];
    const int tid = threadIdx.x, lane = tid & 63;
    const int base = (int)blockIdx.x * SCAN + tid * 4;
    int v[4], s = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        v[j] = base + j < n ? data[base + j] : 0;
        s += v[j];
    }
    int inc = s;                                                // inclusive over the wave
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const int u = __shfl_up(inc, o, 64);
        if (lane >= o) inc += u;
    }
    int off = wave_offsets(__shfl(inc, 63, 64), s_w).x + inc - s;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        if (base + j < n) data[base + j] = off;
        off += v[j];
    }
    if (tid == (int)WG - 1) {
        if (sums) sums[blockIdx.x] = off;
        if (total) *total = off;
    }
}

// list: every root at the position the scan gives it, `first` ascending; the records at keep and beyond are dropped
__global__ __launch_bounds__(256) void k_vzn_list(const int32_t *__restrict__ keys, unsigned dhw, const int *__restrict__ parent,
                                                  const int *__restrict__ size, const int *__restrict__ counts, const int *__restrict__ sums,
                                                  mi_unet_vzone *zones, int keep)
{
    __shared__ int s_n[4];
    const unsigned i = blockIdx.x * WG + threadIdx.x;
    const bool root = is_root(keys, parent, i, dhw);
    const u64 mm = __ballot(root);
    const int pos = counts[blockIdx.x] + sums[blockIdx.x / SCAN] + wave_offsets(__popcll(mm), s_n).x + __popcll(mm & lanes_below());
    const int k = root ? keys[i] : 0, r = (k >> 8) - 1, sz = root ? size[i] : 0;
    if (root && pos < keep) zones[pos] = mi_unet_vzone{ (int32_t)i, r, k & 255, sz };
}

// tally: acc[r].zones and acc[r].largest from every root.  A wave carries a component's count and maximum over consecutive voxels
// (as k_vzn_voxels does): in noise a large component has a root in nearly every voxel, and one atomic per root on its two words would
// be served one after another.
__global__ __launch_bounds__(256) void k_vzn_tally(const int32_t *__restrict__ keys, unsigned dhw, const int *__restrict__ parent,
                                                   const int *__restrict__ size, VznAcc *acc)
{
    const int lane = threadIdx.x & 63;
    const long long first = (((long long)blockIdx.x * WG + threadIdx.x) >> 6) * (64LL * RUN);
    int ar = 0, cnt = 0, big = 0;                               // (wave-uniform) the component number carried (0: none), its roots, its largest
    auto flush = [&]() {
        if (ar && lane == 0) {
            atomicAdd(&acc[ar - 1].zones, cnt);
            raise(&acc[ar - 1].largest, big);
        }
    };
    for (int sg = 0; sg < RUN; ++sg) {
        if (first + 64LL * sg >= (long long)dhw) break;         // (wave-uniform)
        const long long i = first + 64LL * sg + lane;
        int r = 0, sz = 0;
        if (i < (long long)dhw && is_root(keys, parent, (unsigned)i, dhw)) {
            r = keys[i] >> 8;
            sz = size[i];
        }
        peel<GROUPS>(r, 0, [&](int r0, bool mine, u64 mm, int) {
            if (r0 != ar) {
                flush();
                ar = r0; cnt = 0; big = 0;
            }
            cnt += __popcll(mm);
            big = max(big, wave_max(mine ? sz : 0));
        });
        if (r) {                                                // a segment of many small components: the lane adds its own root
            atomicAdd(&acc[r - 1].zones, 1);
            raise(&acc[r - 1].largest, sz);
        }
    }
    flush();
}

// ---- finish: a workgroup per component -----------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_vzn_finish(const int2 *__restrict__ range, int cells, int want, const VznAcc *__restrict__ acc,
                                                    uint32_t *inter, const uint32_t *__restrict__ axial, mi_unet_vzones *table)
{
    __shared__ long long s_sum[2][4];
    const int r = blockIdx.x;
    const bool do_axial = want & VZN_WANT_AXIAL, do_inter = want & VZN_WANT_INTER;
    long long all = 0, ax = 0;
    if (do_axial || do_inter)
        for (int c = threadIdx.x; c < cells; c += WG) {
            const uint32_t va = do_axial ? axial[(size_t)r * cells + c] : 0u;
            ax += va;
            if (do_inter) {
                const uint32_t v = inter[(size_t)r * cells + c] + va;   // (below 13 * 2^28)
                inter[(size_t)r * cells + c] = v;
                all += v;
            }
        }
    all = wave_sum(all); ax = wave_sum(ax);
    if ((threadIdx.x & 63) == 0) {
        s_sum[0][threadIdx.x >> 6] = all; s_sum[1][threadIdx.x >> 6] = ax;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        const int2 rg = range[r];
        const VznAcc c = acc[r];
        mi_unet_vzones t;
        t.voxels = c.voxels;
        t.imin = t.voxels ? 65535 - rg.x : 0;
        t.imax = rg.y;
        t.longest_run = do_inter ? c.longest : 0;
        t.zones = c.zones;
        t.largest_zone = c.largest;
        t.runs = s_sum[0][0] + s_sum[0][1] + s_sum[0][2] + s_sum[0][3];
        t.runs_axial = s_sum[1][0] + s_sum[1][1] + s_sum[1][2] + s_sum[1][3];
        t.clamped = do_inter ? (long long)(c.clamped_axial + c.clamped_inter) : 0;
        t.clamped_axial = (long long)c.clamped_axial;
        table[r] = t;
    }
}

// What the kernels' own arithmetic assumes (the entry points check the arguments and say what is wrong): an index of a voxel and of a
// cell in 32 bits, a component's number and a level in one key.
bool fits(const VolumeZonesArgs &a)
{
    if (a.D < 1 || a.H < 1 || a.W < 1 || (long long)a.D * a.H * a.W > MI_UNET_VTEX_MAX_VOXELS) return false;
    if (a.m < 1 || a.m > MI_UNET_VOLUME_MAX_TABLE || a.L < 1 || a.L > MI_UNET_VTEX_MAX_LEVELS || a.R < 1) return false;
    return (long long)a.m * a.L * a.R <= MI_UNET_VTEX_MAX_CELLS;
}

inline unsigned blocks(unsigned n) { return (n + WG - 1) / WG; }

}  // namespace vzn

size_t vzn_scan_ints(size_t dhw)
{
    const size_t nb = (dhw + vzn::WG - 1) / vzn::WG;
    return nb + (nb + vzn::SCAN - 1) / vzn::SCAN;
}

hipError_t launch_volume_zones_part(const int32_t *ids, const VolumeZonesArgs &a, int first, int count, int32_t *part, hipStream_t s)
{
    if (!ids || !part || !vzn::fits(a) || first < 0 || count < 1 || first + count > a.m) return hipErrorInvalidValue;
    const unsigned dhw = (unsigned)a.D * (unsigned)a.H * (unsigned)a.W;
    hipLaunchKernelGGL(vzn::k_vzn_part, dim3(vzn::blocks(dhw)), dim3(vzn::WG), 0, s, ids, dhw, first, count, part);
    return hipGetLastError();
}

hipError_t launch_volume_zones_join(const int32_t *part, const VolumeZonesArgs &a, int first, int32_t *keys, hipStream_t s)
{
    if (!part || !keys || !vzn::fits(a) || first < 0 || first >= a.m) return hipErrorInvalidValue;
    const unsigned dhw = (unsigned)a.D * (unsigned)a.H * (unsigned)a.W;
    hipLaunchKernelGGL(vzn::k_vzn_join, dim3(vzn::blocks(dhw)), dim3(vzn::WG), 0, s, part, dhw, first, keys);
    return hipGetLastError();
}

hipError_t launch_volume_zones_runs(const int32_t *keys, const VolumeZonesArgs &a, int want, VznAcc *acc, uint32_t *inter, uint32_t *axial,
                                    hipStream_t s)
{
    if (!keys || !acc || !inter || !axial || !vzn::fits(a) || (want & ~(VZN_WANT_AXIAL | VZN_WANT_INTER))) return hipErrorInvalidValue;
    const unsigned dhw = (unsigned)a.D * (unsigned)a.H * (unsigned)a.W;
    const size_t cells = (size_t)a.m * a.L * a.R;
    if (hipError_t e = hipMemsetAsync(acc, 0, (size_t)a.m * sizeof(VznAcc), s)) return e;
    const unsigned waves = (dhw + 64u * vzn::RUN - 1) / (64u * vzn::RUN);
    hipLaunchKernelGGL(vzn::k_vzn_voxels, dim3((waves + 3) / 4), dim3(vzn::WG), 0, s, keys, dhw, acc);
    if (hipError_t e = hipGetLastError()) return e;
    if (!want) return hipSuccess;
    if (want & VZN_WANT_INTER)
        if (hipError_t e = hipMemsetAsync(inter, 0, cells * sizeof(uint32_t), s)) return e;
    if (hipError_t e = hipMemsetAsync(axial, 0, cells * sizeof(uint32_t), s)) return e;
    const int tiles_x = (a.W + vzn::TX - 1) / vzn::TX, tiles_y = (a.H + vzn::TY - 1) / vzn::TY, tiles_z = (a.D + vzn::TZ - 1) / vzn::TZ;
    const int n_tiles = tiles_x * tiles_y * tiles_z;            // (at most 2^21: a side is at most 8192 and the volume 2^28)
    const unsigned grid = (unsigned)((n_tiles + VTX_TILES_PER_WG - 1) / VTX_TILES_PER_WG);
    hipLaunchKernelGGL(vzn::k_vzn_runs, dim3(grid), dim3(vzn::WG), 0, s, keys, a, want, tiles_x, tiles_y, n_tiles, acc, inter, axial);
    return hipGetLastError();
}

hipError_t launch_volume_zones_list(const int32_t *keys, const VolumeZonesArgs &a, int32_t *parent, int32_t *size, int32_t *scan, VznAcc *acc,
                                    ::mi_unet_vzone *zones, int keep_zones, int32_t *found, hipStream_t s)
{
    if (!keys || !parent || !size || !scan || !acc || !zones || !found || keep_zones < 1 || !vzn::fits(a)) return hipErrorInvalidValue;
    const unsigned dhw = (unsigned)a.D * (unsigned)a.H * (unsigned)a.W, nb = vzn::blocks(dhw);
    const int nb1 = (int)((nb + vzn::SCAN - 1) / vzn::SCAN);    // (at most 1024: the upper level is one workgroup)
    if (nb1 > vzn::SCAN) return hipErrorInvalidValue;
    const dim3 g(nb), blk(vzn::WG);
    if (hipError_t e = hipMemsetAsync(size, 0, (size_t)dhw * sizeof(int32_t), s)) return e;
    hipLaunchKernelGGL(vzn::k_vzn_init, g, blk, 0, s, keys, dhw, a.W, parent);
    if (hipError_t e = hipGetLastError()) return e;
    hipLaunchKernelGGL(vzn::k_vzn_merge, g, blk, 0, s, keys, a, dhw, parent);
    if (hipError_t e = hipGetLastError()) return e;
    const unsigned waves = (dhw + 64u * vzn::RUN - 1) / (64u * vzn::RUN);
    hipLaunchKernelGGL(vzn::k_vzn_sizes, dim3((waves + 3) / 4), blk, 0, s, keys, dhw, parent, size);
    if (hipError_t e = hipGetLastError()) return e;
    hipLaunchKernelGGL(vzn::k_vzn_flags, g, blk, 0, s, keys, dhw, parent, scan);
    if (hipError_t e = hipGetLastError()) return e;
    hipLaunchKernelGGL(vzn::k_vzn_scan, dim3((unsigned)nb1), blk, 0, s, scan, (int)nb, scan + nb, (int *)nullptr);
    if (hipError_t e = hipGetLastError()) return e;
    hipLaunchKernelGGL(vzn::k_vzn_scan, dim3(1), blk, 0, s, scan + nb, nb1, (int *)nullptr, found);
    if (hipError_t e = hipGetLastError()) return e;
    hipLaunchKernelGGL(vzn::k_vzn_list, g, blk, 0, s, keys, dhw, parent, size, scan, scan + nb, zones, keep_zones);
    if (hipError_t e = hipGetLastError()) return e;
    hipLaunchKernelGGL(vzn::k_vzn_tally, dim3((waves + 3) / 4), blk, 0, s, keys, dhw, parent, size, acc);
    return hipGetLastError();
}

hipError_t launch_volume_zones_finish(const int2 *range, const VolumeZonesArgs &a, int want, const VznAcc *acc, uint32_t *inter,
                                      const uint32_t *axial, ::mi_unet_vzones *table, hipStream_t s)
{
    if (!range || !acc || !inter || !axial || !table || !vzn::fits(a)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(vzn::k_vzn_finish, dim3((unsigned)a.m), dim3(vzn::WG), 0, s, range, a.L * a.R, want, acc, inter, axial, table);
    return hipGetLastError();
}

}  // namespace miunet
