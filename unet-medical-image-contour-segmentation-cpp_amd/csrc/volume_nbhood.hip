// volume_nbhood.hip -- per component of a labelled stack its neighbourhood-difference, dependence and distance-zone tables
// (include/mi_unet.h: mi_unet_volume_nbhood), on the key stack that volume_texture.hip's launch_volume_texture_keys makes
// and, for the zones, on the forest that volume_zones.hip's launch_volume_zones_list leaves.  k_vnb_gather, the hot path: a tile of keys
// with its full halo in LDS, a lane per voxel reads its 26 neighbours there; the lanes of a wave that name one cell merge before the
// atomic.  k_vnb_dist_x / _y / _z: the multi-label city-block distance transform, one axis after the other; along x a wave per row with
// segmented scans, along y and z a lane per column.  k_vnb_zone_min: the minimum of both distances per root, the maximum per component.
// k_vnb_zone_tally: one count per root into the distance-zone tables.  k_vnb_finish: the table entries.  Every result is an integer
// sum, minimum or maximum, so nothing depends on the order in which atomics arrive; no workgroup waits for another.
// gfx950 only.
#include "../../include/mi_unet.h"
#include "cc_common.h"
#include "kernel_common.h"
#include "kernels.h"
#include "key_tile.h"
#include "wave.h"

namespace miunet {

namespace vnb {

using namespace wave;
using namespace key_tile;

constexpr unsigned WG = 256;                // lanes per workgroup
constexpr int MERGE = 3;                    // distinct cells of one table that a wave merges; lanes beyond them add their own
constexpr int GROUPS = 4;                   // distinct roots of a 64-voxel segment that are reduced across the wave
constexpr int KZ = TZ + 2;                  // key_tile.h's tile with its full halo: z - 1 .. z + 1
constexpr int TILE_KEYS = KX * KY * KZ;     // 3960 keys, 15 840 bytes
constexpr int FAR = 0x7f7f7f7f;             // what hipMemsetAsync(.., 0x7f, ..) leaves: above every distance
// Every count goes through wave.h's merged_add; with `sums` a lane's `val` is below 2^11.

// ---- the neighbourhoods: the hot path -----------------------------------------------------------------------------------------------------
// LDS: the keys of the tile with its halo; a position outside the volume holds 0, which is no neighbour of anything.  A workgroup takes
// VTX_TILES_PER_WG tiles that follow each other along x.  Every key is fetched from memory once per tile.  With LDS_TABLE the six tables
// of one component follow the keys: count, diff and dep of 27 columns, then of 9, L rows each, the diff in 32 bits (a workgroup's
// 8 x 2048 voxels add less than 2^25 to a cell).  That component is the one of the first voxel of the tile (in lane order) that belongs
// to any (as in k_vtx_pairs); when it differs from the tables' owner and holds LDS_SHARE voxels of the tile, the tables are flushed, only
// their non-zero cells, cleared, and are its own from then on.  Counts of every other component of the tile go to memory.
constexpr int NO_PICK = 0x7fffffff;
constexpr int LDS_COLS = 3 * VNB_COLS + 3 * VNB_COLS_AXIAL;    // words a level in the LDS tables
constexpr int LDS_SHARE = 256;                                 // voxels of a tile (of 2048) a component needs to take the LDS tables over

template <bool LDS_TABLE>
__global__ __launch_bounds__(256) void k_vnb_gather(const int32_t *__restrict__ keys, VolumeNbhoodArgs a, int want, int tiles_x, int tiles_y,
                                                    int n_tiles, VnbTables t)
{
    extern __shared__ int s_mem[];
    __shared__ int s_pick, s_share;
    int *const s_keys = s_mem;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int L = a.L, alpha = a.alpha;
    uint32_t *const s_count = reinterpret_cast<uint32_t *>(s_mem + TILE_KEYS);
    uint32_t *const s_diff = s_count + L * VNB_COLS, *const s_dep = s_diff + L * VNB_COLS;
    uint32_t *const s_count_a = s_dep + L * VNB_COLS, *const s_diff_a = s_count_a + L * VNB_COLS_AXIAL, *const s_dep_a = s_diff_a + L * VNB_COLS_AXIAL;
    int owned = 0;                                              // (uniform) the component number (r + 1) whose counts the LDS tables hold
    if (LDS_TABLE)
        for (int c = tid; c < L * LDS_COLS; c += WG) s_count[c] = 0u;
    auto flush = [&]() {                                        // (all lanes; the tables are at rest)
        const size_t row = (size_t)(owned - 1) * L;
        for (int c = tid; c < L * VNB_COLS; c += WG) {
            const uint32_t vc = s_count[c], vd = s_diff[c], vk = s_dep[c];
            if (vc) { atomicAdd(t.count + row * VNB_COLS + c, vc); s_count[c] = 0u; }
            if (vd) { atomicAdd(t.diff + row * VNB_COLS + c, (u64)vd); s_diff[c] = 0u; }
            if (vk) { atomicAdd(t.dep + row * VNB_COLS + c, vk); s_dep[c] = 0u; }
        }
        for (int c = tid; c < L * VNB_COLS_AXIAL; c += WG) {
            const uint32_t vc = s_count_a[c], vd = s_diff_a[c], vk = s_dep_a[c];
            if (vc) { atomicAdd(t.count_axial + row * VNB_COLS_AXIAL + c, vc); s_count_a[c] = 0u; }
            if (vd) { atomicAdd(t.diff_axial + row * VNB_COLS_AXIAL + c, (u64)vd); s_diff_a[c] = 0u; }
            if (vk) { atomicAdd(t.dep_axial + row * VNB_COLS_AXIAL + c, vk); s_dep_a[c] = 0u; }
        }
    };
    const int t_end = min(n_tiles, ((int)blockIdx.x + 1) * VTX_TILES_PER_WG);
    for (int tile = (int)blockIdx.x * VTX_TILES_PER_WG; tile < t_end; ++tile) {
        __syncthreads();                                        // the tile before is done with s_keys and s_pick
        load_key_tile<KZ, 1>(s_keys, keys, tile_origin<1>(tile, tiles_x, tiles_y), a.D, a.H, a.W);
        if (LDS_TABLE) {
            if (tid == 0) {
                s_pick = NO_PICK;
                s_share = 0;
            }
            __syncthreads();
            // the lane's voxels: row = wave * (ROWS / 4) + it of the tile, column = lane
            int pick = NO_PICK;
#pragma unroll
            for (int it = ROWS / 4 - 1; it >= 0; --it) {
                const int row = wave * (ROWS / 4) + it;
                const int k = s_keys[(row / TY + 1) * (KX * KY) + (row % TY + 1) * KX + 1 + lane];
                if (k) pick = (((it * 4 + wave) * 64 + lane) << 13) | (k >> 8);
            }
            if (pick != NO_PICK) atomicMin(&s_pick, pick);
            __syncthreads();
            const int lead = s_pick == NO_PICK ? 0 : (s_pick & 0x1FFF);
            if (lead == 0) continue;                            // (uniform) no voxel of any component in the tile
            if (lead != owned) {
                // the leader takes the tables over only where it holds LDS_SHARE voxels of the tile: a flush sends L * 108 cells through
                // the workgroup, what a few rows of voxels cost, and a component of fewer voxels cannot repay it (a tile of many small
                // components then counts straight to memory, and the tables stay with their owner)
                int mine = 0;
#pragma unroll
                for (int it = 0; it < ROWS / 4; ++it) {
                    const int row = wave * (ROWS / 4) + it;
                    mine += (s_keys[(row / TY + 1) * (KX * KY) + (row % TY + 1) * KX + 1 + lane] >> 8) == lead;
                }
                mine = (int)wave_sum((unsigned)mine);
                if (lane == 0) atomicAdd(&s_share, mine);
                __syncthreads();
                if (s_share >= LDS_SHARE) {                     // (uniform)
                    if (owned) flush();
                    owned = lead;
                    __syncthreads();
                }
            }
        } else {
            __syncthreads();
        }
#pragma unroll 1
        for (int it = 0; it < ROWS / 4; ++it) {
            const int row = wave * (ROWS / 4) + it;
            const int lz = row / TY + 1, ly = row % TY + 1, lx = lane + 1;
            const int *const p = s_keys + lz * (KX * KY) + ly * KX + lx;
            const int k = *p;
            if (!__ballot(k != 0)) continue;                    // (wave-uniform) a row of no component
            const int id = k >> 8, l = k & 255;
            int c8 = 0, s8 = 0, k8 = 0, c18 = 0, s18 = 0, k18 = 0;              // over the 8 with dz = 0 and over the 18 others
#pragma unroll
            for (int dz = -1; dz <= 1; ++dz)
#pragma unroll
                for (int dy = -1; dy <= 1; ++dy)
#pragma unroll
                    for (int dx = -1; dx <= 1; ++dx) {
                        if (dx == 0 && dy == 0 && dz == 0) continue;
                        const int q = p[dz * (KX * KY) + dy * KX + dx];
                        const int same = (q >> 8) == id;        // (id is at least 1 where it matters, so a 0 is never the same)
                        const int ql = q & 255;
                        const int near = same && abs(ql - l) <= alpha;
                        if (dz == 0) {
                            c8 += same; s8 += same ? ql : 0; k8 += near;
                        } else {
                            c18 += same; s18 += same ? ql : 0; k18 += near;
                        }
                    }
            const int c26 = c8 + c18, s26 = s8 + s18, k26 = k8 + k18;
            const unsigned d26 = (unsigned)abs(c26 * l - s26), d8 = (unsigned)abs(c8 * l - s8);
            const bool in_lds = LDS_TABLE && k != 0 && id == owned;
            const bool in_mem = k != 0 && !in_lds;
            const unsigned base = (unsigned)(id - 1) * (unsigned)L + (unsigned)l;           // (below 2^17; only used when k != 0)
            uint32_t *const none = nullptr;
            if (want & VNB_WANT_NGT) {
                if (LDS_TABLE) merged_add<MERGE>(s_count, s_diff, in_lds, (unsigned)(l * VNB_COLS + c26), d26);
                merged_add<MERGE>(t.count, t.diff, in_mem, base * VNB_COLS + (unsigned)c26, d26);
            }
            if (want & VNB_WANT_DEP) {
                if (LDS_TABLE) merged_add<MERGE>(s_dep, none, in_lds, (unsigned)(l * VNB_COLS + k26), 0u);
                merged_add<MERGE>(t.dep, none, in_mem, base * VNB_COLS + (unsigned)k26, 0u);
            }
            if (want & VNB_WANT_NGT_AXIAL) {
                if (LDS_TABLE) merged_add<MERGE>(s_count_a, s_diff_a, in_lds, (unsigned)(l * VNB_COLS_AXIAL + c8), d8);
                merged_add<MERGE>(t.count_axial, t.diff_axial, in_mem, base * VNB_COLS_AXIAL + (unsigned)c8, d8);
            }
            if (want & VNB_WANT_DEP_AXIAL) {
                if (LDS_TABLE) merged_add<MERGE>(s_dep_a, none, in_lds, (unsigned)(l * VNB_COLS_AXIAL + k8), 0u);
                merged_add<MERGE>(t.dep_axial, none, in_mem, base * VNB_COLS_AXIAL + (unsigned)k8, 0u);
            }
        }
    }
    if (LDS_TABLE && owned) {
        __syncthreads();
        flush();
    }
}

// ---- the distance transform ---------------------------------------------------------------------------------------------------------------
// Along x: the distance of a voxel to the nearest end of its run of one component inside its row, both ends counted from 1 (the position
// beyond an end is of another component or outside the volume).  A wave per row; forward in chunks of 64 it carries the start of the run
// that is open, backward its end.  Voxels of no component are measured like a component of their own; nobody reads their values.
__global__ __launch_bounds__(256) void k_vnb_dist_x(const int32_t *__restrict__ keys, int W, unsigned rows, uint16_t *dist)
{
    const int lane = threadIdx.x & 63;
    const unsigned row = blockIdx.x * (WG / 64) + (threadIdx.x >> 6);
    if (row >= rows) return;                                    // (wave-uniform)
    const int32_t *const krow = keys + (size_t)row * W;
    uint16_t *const drow = dist + (size_t)row * W;
    const int chunks = (W + 63) / 64;
    int carry_start = 0, carry_comp = -2;
    for (int ch = 0; ch < chunks; ++ch) {
        const int x = ch * 64 + lane;
        const int comp = x < W ? krow[x] >> 8 : -1;
        int prev = __shfl_up(comp, 1, 64);
        if (lane == 0) prev = carry_comp;
        int start = comp != prev ? x : -1;                      // the start of the run this voxel belongs to: the largest start at or before it
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const int u = __shfl_up(start, o, 64);
            if (lane >= o) start = max(start, u);
        }
        start = max(start, carry_start);
        if (x < W) drow[x] = (uint16_t)(x - start + 1);
        carry_start = __shfl(start, 63, 64);
        carry_comp = __shfl(comp, 63, 64);
    }
    int carry_end = W - 1;
    carry_comp = -2;
    for (int ch = chunks - 1; ch >= 0; --ch) {
        const int x = ch * 64 + lane;
        const int comp = x < W ? krow[x] >> 8 : -1;
        int next = __shfl_down(comp, 1, 64);
        if (lane == 63) next = carry_comp;
        int end = (comp != next || x == W - 1) ? x : 0x7fffffff;        // the smallest end at or behind the voxel
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const int u = __shfl_down(end, o, 64);
            if (lane + o < 64) end = min(end, u);
        }
        end = min(end, carry_end);
        if (x < W) drow[x] = (uint16_t)min((int)drow[x], end - x + 1);          // (the lane reads what it wrote itself)
        carry_end = __shfl(end, 0, 64);
        carry_comp = __shfl(comp, 0, 64);
    }
}

// Along y (stride = W, n = H, a column per (z, x)) and along z (stride = H W, n = D, a column per (y, x)): forward, then backward,
//     carry = component(previous) == component(this) ? value(previous) + 1 : 1;  value = min(value, carry);
// the first voxel of a column gets carry 1.  `in` holds the values of the axes before, `out` takes the result; they may be the same.
__global__ __launch_bounds__(256) void k_vnb_dist_col(const int32_t *__restrict__ keys, int n, size_t stride, unsigned per_slab, size_t slab_stride,
                                                      const uint16_t *in, uint16_t *out)
{
    const unsigned c = blockIdx.x * WG + threadIdx.x;
    if (c >= per_slab) return;
    const size_t first = (size_t)blockIdx.y * slab_stride + c;
    int prev_comp = -2, prev_val = 0;
    for (int j = 0; j < n; ++j) {
        const size_t i = first + (size_t)j * stride;
        const int comp = keys[i] >> 8;
        const int v = min((int)in[i], comp == prev_comp ? prev_val + 1 : 1);
        out[i] = (uint16_t)v;
        prev_comp = comp; prev_val = v;
    }
    prev_comp = -2;
    for (int j = n - 1; j >= 0; --j) {
        const size_t i = first + (size_t)j * stride;
        const int comp = keys[i] >> 8;
        const int v = min((int)out[i], comp == prev_comp ? prev_val + 1 : 1);
        out[i] = (uint16_t)v;
        prev_comp = comp; prev_val = v;
    }
}

// ---- the zones' distances -------------------------------------------------------------------------------------------------------------------
// zone_min: zmin[root] and zmin_axial[root] = the minimum over the zone (both preset to FAR), acc[r].deepest(_axial) = the maximum over the
// component.  The voxels of a 64-lane segment that share a root merge first, for the first GROUPS roots.
__global__ __launch_bounds__(256) void k_vnb_zone_min(const int32_t *__restrict__ keys, unsigned dhw, const int *parent, const uint16_t *__restrict__ axial,
                                                      const uint16_t *__restrict__ full, int *zmin, int *zmin_axial, VnbAcc *acc)
{
    const unsigned i = blockIdx.x * WG + threadIdx.x;
    const int lane = threadIdx.x & 63;
    const int k = i < dhw ? keys[i] : 0;
    int root = -1, da = 0, df = 0;
    if (k) {
        root = pp::find_root_ro(parent, (int)i);
        if (axial) da = axial[i];
        if (full) df = full[i];
    }
    const int comp = k >> 8;
    peel<GROUPS>(root, -1, [&](int r0, bool mine, u64, int leader) {
        if (axial) {                                            // (wave-uniform)
            const int lo = wave_min(mine ? da : FAR), hi = wave_max(mine ? da : 0);
            if (lane == leader) {
                lower(zmin_axial + r0, lo);
                raise(&acc[comp - 1].deepest_axial, hi);
            }
        }
        if (full) {
            const int lo = wave_min(mine ? df : FAR), hi = wave_max(mine ? df : 0);
            if (lane == leader) {
                lower(zmin + r0, lo);
                raise(&acc[comp - 1].deepest, hi);
            }
        }
    });
    if (root >= 0) {
        if (axial) {
            lower(zmin_axial + root, da);
            raise(&acc[comp - 1].deepest_axial, da);
        }
        if (full) {
            lower(zmin + root, df);
            raise(&acc[comp - 1].deepest, df);
        }
    }
}

// zone_tally: every root adds its zone to cell (r, level, min(distance, Dm) - 1) of the tables that are wanted
__global__ __launch_bounds__(256) void k_vnb_zone_tally(const int32_t *__restrict__ keys, unsigned dhw, const int *__restrict__ parent, int L, int Dm,
                                                        const int *__restrict__ zmin, const int *__restrict__ zmin_axial, VnbAcc *acc, uint32_t *dzm,
                                                        uint32_t *dzm_axial)
{
    const unsigned i = blockIdx.x * WG + threadIdx.x;
    const int k = i < dhw ? keys[i] : 0;
    const bool root = k != 0 && parent[i] == (int)i;
    if (!__ballot(root)) return;                                // (wave-uniform)
    const unsigned r = root ? (unsigned)(k >> 8) - 1u : 0u;
    const unsigned base = (r * (unsigned)L + (unsigned)(k & 255)) * (unsigned)Dm;           // (below 2^22)
    uint32_t *const words = reinterpret_cast<uint32_t *>(acc);  // (VnbAcc is four words; clamped is word 2, clamped_axial word 3)
    if (dzm) {                                                  // (wave-uniform)
        const int d = root ? max(zmin[i], 1) : 1;
        merged_add<MERGE>(dzm, (uint32_t *)nullptr, root, base + (unsigned)(min(d, Dm) - 1), 0u);
        merged_add<MERGE>(words, (uint32_t *)nullptr, root && d > Dm, r * 4u + 2u, 0u);
    }
    if (dzm_axial) {
        const int d = root ? max(zmin_axial[i], 1) : 1;
        merged_add<MERGE>(dzm_axial, (uint32_t *)nullptr, root, base + (unsigned)(min(d, Dm) - 1), 0u);
        merged_add<MERGE>(words, (uint32_t *)nullptr, root && d > Dm, r * 4u + 3u, 0u);
    }
}

// ---- finish: a workgroup per component -----------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_vnb_finish(const int2 *__restrict__ range, int L, int want, const VznAcc *__restrict__ zacc,
                                                    const VnbAcc *__restrict__ acc, VnbTables t, mi_unet_vnbhood *table)
{
    __shared__ int s_v[3][4];
    const int r = blockIdx.x;
    int valid = 0, valid_axial = 0, dep_max = 0;                // (a component has at most 2^28 voxels)
    if (want & VNB_WANT_NGT)
        for (int c = threadIdx.x; c < L * VNB_COLS; c += WG)
            if (c % VNB_COLS) valid += (int)t.count[(size_t)r * L * VNB_COLS + c];
    if (want & VNB_WANT_NGT_AXIAL)
        for (int c = threadIdx.x; c < L * VNB_COLS_AXIAL; c += WG)
            if (c % VNB_COLS_AXIAL) valid_axial += (int)t.count_axial[(size_t)r * L * VNB_COLS_AXIAL + c];
    if (want & VNB_WANT_DEP)
        for (int c = threadIdx.x; c < L * VNB_COLS; c += WG)
            if (t.dep[(size_t)r * L * VNB_COLS + c]) dep_max = max(dep_max, c % VNB_COLS + 1);
    valid = (int)wave_sum((unsigned)valid); valid_axial = (int)wave_sum((unsigned)valid_axial); dep_max = wave_max(dep_max);
    if ((threadIdx.x & 63) == 0) {
        s_v[0][threadIdx.x >> 6] = valid; s_v[1][threadIdx.x >> 6] = valid_axial; s_v[2][threadIdx.x >> 6] = dep_max;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        const int2 rg = range[r];
        const VznAcc z = zacc[r];
        const VnbAcc c = acc[r];
        const bool zones = want & (VNB_WANT_DZM | VNB_WANT_DZM_AXIAL);
        mi_unet_vnbhood e;
        e.voxels = z.voxels;
        e.imin = e.voxels ? 65535 - rg.x : 0;
        e.imax = rg.y;
        e.valid = s_v[0][0] + s_v[0][1] + s_v[0][2] + s_v[0][3];
        e.valid_axial = s_v[1][0] + s_v[1][1] + s_v[1][2] + s_v[1][3];
        e.zones = zones ? z.zones : 0;
        e.deepest = (want & VNB_WANT_DZM) ? c.deepest : 0;
        e.deepest_axial = (want & VNB_WANT_DZM_AXIAL) ? c.deepest_axial : 0;
        e.clamped = (want & VNB_WANT_DZM) ? (int)c.clamped : 0;
        e.clamped_axial = (want & VNB_WANT_DZM_AXIAL) ? (int)c.clamped_axial : 0;
        e.dependence_max = max(max(s_v[2][0], s_v[2][1]), max(s_v[2][2], s_v[2][3]));
        table[r] = e;
    }
}

// What the kernels' own arithmetic assumes (the entry points check the arguments and say what is wrong): an index of a voxel and of a
// cell in 32 bits, a component's number and a level in one key.
bool fits(const VolumeNbhoodArgs &a)
{
    if (a.D < 1 || a.H < 1 || a.W < 1 || a.D > MI_UNET_SCORE_VOLUME_MAX_SIDE || a.H > MI_UNET_SCORE_VOLUME_MAX_SIDE || a.W > MI_UNET_SCORE_VOLUME_MAX_SIDE)
        return false;
    if ((long long)a.D * a.H * a.W > MI_UNET_VTEX_MAX_VOXELS) return false;
    if (a.m < 1 || a.m > MI_UNET_VOLUME_MAX_TABLE || a.L < 1 || a.L > MI_UNET_VTEX_MAX_LEVELS) return false;
    if (a.alpha < 0 || a.Dm < 1 || a.Dm > MI_UNET_VNBHOOD_MAX_DIST) return false;
    const int widest = a.Dm > 32 ? (a.Dm > a.L ? a.Dm : a.L) : (a.L > 32 ? a.L : 32);
    return (long long)a.m * a.L * widest <= MI_UNET_VTEX_MAX_CELLS;
}

inline unsigned blocks(unsigned n) { return (n + WG - 1) / WG; }

}  // namespace vnb

hipError_t launch_volume_nbhood_gather(const int32_t *keys, const VolumeNbhoodArgs &a, int want, bool lds_table, const VnbTables &t, hipStream_t s)
{
    if (!keys || !vnb::fits(a)) return hipErrorInvalidValue;
    if (((want & VNB_WANT_NGT) && (!t.count || !t.diff)) || ((want & VNB_WANT_DEP) && !t.dep) ||
        ((want & VNB_WANT_NGT_AXIAL) && (!t.count_axial || !t.diff_axial)) || ((want & VNB_WANT_DEP_AXIAL) && !t.dep_axial))
        return hipErrorInvalidValue;
    const size_t rows = (size_t)a.m * a.L;
    if (want & VNB_WANT_NGT) {
        if (hipError_t e = hipMemsetAsync(t.count, 0, rows * VNB_COLS * sizeof(uint32_t), s)) return e;
        if (hipError_t e = hipMemsetAsync(t.diff, 0, rows * VNB_COLS * sizeof(unsigned long long), s)) return e;
    }
    if (want & VNB_WANT_DEP)
        if (hipError_t e = hipMemsetAsync(t.dep, 0, rows * VNB_COLS * sizeof(uint32_t), s)) return e;
    if (want & VNB_WANT_NGT_AXIAL) {
        if (hipError_t e = hipMemsetAsync(t.count_axial, 0, rows * VNB_COLS_AXIAL * sizeof(uint32_t), s)) return e;
        if (hipError_t e = hipMemsetAsync(t.diff_axial, 0, rows * VNB_COLS_AXIAL * sizeof(unsigned long long), s)) return e;
    }
    if (want & VNB_WANT_DEP_AXIAL)
        if (hipError_t e = hipMemsetAsync(t.dep_axial, 0, rows * VNB_COLS_AXIAL * sizeof(uint32_t), s)) return e;
    if (!(want & (VNB_WANT_NGT | VNB_WANT_DEP | VNB_WANT_NGT_AXIAL | VNB_WANT_DEP_AXIAL))) return hipSuccess;
    const int tiles_x = (a.W + vnb::TX - 1) / vnb::TX, tiles_y = (a.H + vnb::TY - 1) / vnb::TY, tiles_z = (a.D + vnb::TZ - 1) / vnb::TZ;
    const int n_tiles = tiles_x * tiles_y * tiles_z;            // (at most 2^21: a side is at most 8192 and the volume 2^28)
    const unsigned grid = (unsigned)((n_tiles + VTX_TILES_PER_WG - 1) / VTX_TILES_PER_WG);
    const size_t keys_bytes = (size_t)vnb::TILE_KEYS * sizeof(int);
    if (lds_table)
        hipLaunchKernelGGL(vnb::k_vnb_gather<true>, dim3(grid), dim3(vnb::WG), keys_bytes + (size_t)a.L * vnb::LDS_COLS * sizeof(uint32_t), s, keys, a,
                           want, tiles_x, tiles_y, n_tiles, t);
    else
        hipLaunchKernelGGL(vnb::k_vnb_gather<false>, dim3(grid), dim3(vnb::WG), keys_bytes, s, keys, a, want, tiles_x, tiles_y, n_tiles, t);
    return hipGetLastError();
}

hipError_t launch_volume_nbhood_dist(const int32_t *keys, const VolumeNbhoodArgs &a, uint16_t *axial, uint16_t *full, hipStream_t s)
{
    if (!keys || !axial || !vnb::fits(a)) return hipErrorInvalidValue;
    const unsigned rows = (unsigned)a.D * (unsigned)a.H;        // (at most 2^28)
    hipLaunchKernelGGL(vnb::k_vnb_dist_x, dim3((rows + 3) / 4), dim3(vnb::WG), 0, s, keys, a.W, rows, axial);
    if (hipError_t e = hipGetLastError()) return e;
    const size_t hw = (size_t)a.H * a.W;
    // along y: a slab is a slice (the grid's y is at most 8192), a column per x
    hipLaunchKernelGGL(vnb::k_vnb_dist_col, dim3(vnb::blocks((unsigned)a.W), (unsigned)a.D), dim3(vnb::WG), 0, s, keys, a.H, (size_t)a.W, (unsigned)a.W, hw,
                       (const uint16_t *)axial, axial);
    if (hipError_t e = hipGetLastError()) return e;
    if (!full) return hipSuccess;
    // along z: one slab, a column per (y, x)
    hipLaunchKernelGGL(vnb::k_vnb_dist_col, dim3(vnb::blocks((unsigned)hw), 1u), dim3(vnb::WG), 0, s, keys, a.D, hw, (unsigned)hw, (size_t)0,
                       (const uint16_t *)axial, full);
    return hipGetLastError();
}

hipError_t launch_volume_nbhood_zones(const int32_t *keys, const VolumeNbhoodArgs &a, int want, const int32_t *parent, const uint16_t *axial,
                                      const uint16_t *full, int32_t *zmin, int32_t *zmin_axial, VnbAcc *acc, const VnbTables &t, hipStream_t s)
{
    const bool do_full = want & VNB_WANT_DZM, do_axial = want & VNB_WANT_DZM_AXIAL;
    if (!keys || !parent || !acc || !vnb::fits(a) || (!do_full && !do_axial)) return hipErrorInvalidValue;
    if ((do_full && (!full || !zmin || !t.dzm)) || (do_axial && (!axial || !zmin_axial || !t.dzm_axial))) return hipErrorInvalidValue;
    const unsigned dhw = (unsigned)a.D * (unsigned)a.H * (unsigned)a.W;
    const size_t cells = (size_t)a.m * a.L * a.Dm;
    if (hipError_t e = hipMemsetAsync(acc, 0, (size_t)a.m * sizeof(VnbAcc), s)) return e;
    if (do_full) {
        if (hipError_t e = hipMemsetAsync(zmin, 0x7f, (size_t)dhw * sizeof(int32_t), s)) return e;
        if (hipError_t e = hipMemsetAsync(t.dzm, 0, cells * sizeof(uint32_t), s)) return e;
    }
    if (do_axial) {
        if (hipError_t e = hipMemsetAsync(zmin_axial, 0x7f, (size_t)dhw * sizeof(int32_t), s)) return e;
        if (hipError_t e = hipMemsetAsync(t.dzm_axial, 0, cells * sizeof(uint32_t), s)) return e;
    }
    const dim3 g(vnb::blocks(dhw)), blk(vnb::WG);
    hipLaunchKernelGGL(vnb::k_vnb_zone_min, g, blk, 0, s, keys, dhw, parent, do_axial ? axial : (const uint16_t *)nullptr,
                       do_full ? full : (const uint16_t *)nullptr, zmin, zmin_axial, acc);
    if (hipError_t e = hipGetLastError()) return e;
    hipLaunchKernelGGL(vnb::k_vnb_zone_tally, g, blk, 0, s, keys, dhw, parent, a.L, a.Dm, (const int *)zmin, (const int *)zmin_axial, acc,
                       do_full ? t.dzm : (uint32_t *)nullptr, do_axial ? t.dzm_axial : (uint32_t *)nullptr);
    return hipGetLastError();
}

hipError_t launch_volume_nbhood_finish(const int2 *range, const VolumeNbhoodArgs &a, int want, const VznAcc *zacc, const VnbAcc *acc,
                                       const VnbTables &t, ::mi_unet_vnbhood *table, hipStream_t s)
{
    if (!range || !zacc || !acc || !table || !vnb::fits(a)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(vnb::k_vnb_finish, dim3((unsigned)a.m), dim3(vnb::WG), 0, s, range, a.L, want, zacc, acc, t, table);
    return hipGetLastError();
}

}  // namespace miunet
