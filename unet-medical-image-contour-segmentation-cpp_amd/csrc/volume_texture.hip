// volume_texture.hip -- per component of a labelled stack its grey-level histogram and its 3-D co-occurrence tables (include/mi_unet.h:
// mi_unet_volume_texture).  k_vtx_range: a lane per voxel, the wave reduces per distinct id and carries an id's
// minimum and maximum until the id changes (wave.h's peel).  k_vtx_keys: ids in place into (r + 1) << 8 | level.  k_vtx_pairs, the
// hot path: a tile of keys with its halo in LDS, the 13 forward neighbours of every voxel compared there, the counts of the component
// that leads the tile kept in LDS-private tables.  k_vtx_finish: the 13-offset table from its two parts, and the table entries.  Every
// result is an integer sum, minimum or maximum, so nothing depends on the order in which atomics arrive; no workgroup waits for another.
// gfx950 only.
#include "../../include/mi_unet.h"
#include "kernel_common.h"
#include "kernels.h"
#include "key_tile.h"
#include "wave.h"

namespace miunet {

namespace vtx {

using namespace wave;
using namespace key_tile;

constexpr unsigned WG = 256;                // lanes per workgroup
constexpr int RUN = 16;                     // 64-voxel segments a wave of k_vtx_range carries an id over
constexpr int GROUPS = 4;                   // distinct ids of a segment that are reduced across the wave; lanes beyond them add their own
constexpr int MERGE = 3;                    // distinct cells of one offset that a wave of k_vtx_pairs merges; lanes beyond them add their own
constexpr int KZ = TZ + 1;                  // key_tile.h's tile with the slice behind it: z .. z + 1
constexpr int TILE_KEYS = KX * KY * KZ;
constexpr int NO_PICK = 0x7FFFFFFF;
static_assert(MI_UNET_VOLUME_MAX_TABLE < (1 << 13), "a pick holds a component's number in 13 bits");

// ---- range: 65535 - imin and imax per component; one lane per voxel ---------------------------------------------------------------------------
// Both only grow: wave.h's raise.
__global__ __launch_bounds__(256) void k_vtx_range(const int32_t *__restrict__ ids, const uint16_t *__restrict__ inten, unsigned dhw, int m,
                                                   int2 *range)
{
    const int lane = threadIdx.x & 63;
    const long long first = (((long long)blockIdx.x * WG + threadIdx.x) >> 6) * (64LL * RUN);
    int ar = -1, lo = 65535, hi = 0;                            // (wave-uniform) the id carried, and its minimum and maximum
    auto flush = [&]() {
        if (ar < 0) return;
        int *const c = reinterpret_cast<int *>(range + ar);
        if (lane == 0) raise(c, 65535 - lo);                    // (turned round: 0 = no voxel yet)
        else if (lane == 1) raise(c + 1, hi);
    };
    for (int sg = 0; sg < RUN; ++sg) {
        if (first + 64LL * sg >= (long long)dhw) break;         // (wave-uniform)
        const long long i = first + 64LL * sg + lane;
        int r = -1, v = 0;
        if (i < (long long)dhw) {
            const int id = ids[i];
            if (id >= 1 && id <= m) {
                r = id - 1;
                v = inten[i];
            }
        }
        peel<GROUPS>(r, -1, [&](int r0, bool mine, u64, int) {
            if (r0 != ar) {
                flush();
                ar = r0; lo = 65535; hi = 0;
            }
            lo = min(lo, wave_min(mine ? v : 65535));
            hi = max(hi, wave_max(mine ? v : 0));
        });
        if (r >= 0) {                                           // a segment of many small components: the lane adds its own voxel
            int *const c = reinterpret_cast<int *>(range + r);
            raise(c, 65535 - v);
            raise(c + 1, v);
        }
    }
    flush();
}

// ---- keys: ids in place into (r + 1) << 8 | level, 0 for a voxel of no component ---------------------------------------------------------------
__global__ __launch_bounds__(256) void k_vtx_keys(int32_t *__restrict__ ids, const uint16_t *__restrict__ inten, unsigned dhw,
                                                  VolumeTextureArgs a, const int2 *__restrict__ range)
{
    const unsigned i = blockIdx.x * WG + threadIdx.x;
    if (i >= dhw) return;
    const int id = ids[i];
    int key = 0;
    if (id >= 1 && id <= a.m) {
        const unsigned v = inten[i];
        unsigned level;
        if (a.mode == MI_UNET_VTEX_COUNT) {
            const int2 rg = range[id - 1];
            const unsigned imin = 65535u - (unsigned)rg.x, imax = (unsigned)rg.y;
            level = ((v - imin) * (unsigned)a.L) / (imax - imin + 1u);          // (below 2^16 * 2^6; v - imin <= imax - imin, so below L)
        } else {
            level = v < (unsigned)a.lo ? 0u : min((unsigned)a.L - 1u, (v - (unsigned)a.lo) / (unsigned)a.width);
        }
        key = (id << 8) | (int)level;
    }
    ids[i] = key;
}

// ---- pairs: the hot path -------------------------------------------------------------------------------------------------------------------
// Every count goes through wave.h's merged_add: into a table in LDS or in memory (where the cell also names the component).
// LDS: the keys of the tile with its halo, then (LDS_TABLE) the owned component's axial table [L][L], inter table [L][L] and
// histogram [L].  A workgroup takes VTX_TILES_PER_WG tiles that follow each other along x.  The component that owns the LDS tables is
// the one of the first voxel of the tile (in lane order) that belongs to any; when it differs from the tile before, the tables are
// flushed, only their non-zero cells, and cleared.  Counts of every other component of the tile go to memory.
template <bool LDS_TABLE>
__global__ __launch_bounds__(256) void k_vtx_pairs(const int32_t *__restrict__ keys, VolumeTextureArgs a, int want, int tiles_x, int tiles_y,
                                                   int n_tiles, uint32_t *hist, uint32_t *inter, uint32_t *axial)
{
    extern __shared__ int s_mem[];
    __shared__ int s_pick;
    int *const s_keys = s_mem;
    const int L = a.L, LL = L * L;
    uint32_t *const s_axial = reinterpret_cast<uint32_t *>(s_mem + TILE_KEYS);
    uint32_t *const s_inter = s_axial + LL;
    uint32_t *const s_hist = s_inter + LL;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const bool do_axial = want & VTX_WANT_AXIAL, do_inter = want & VTX_WANT_INTER;
    int owned = 0;                                              // (uniform) the component number (r + 1) whose counts the LDS tables hold
    if (LDS_TABLE)
        for (int c = tid; c < 2 * LL + L; c += WG) s_axial[c] = 0u;
    auto flush = [&]() {                                        // (all lanes; the tables are at rest)
        const size_t base = (size_t)(owned - 1) * LL;
        for (int c = tid; c < LL; c += WG) {
            const uint32_t va = s_axial[c], vi = s_inter[c];
            if (va) { atomicAdd(axial + base + c, va); s_axial[c] = 0u; }
            if (vi) { atomicAdd(inter + base + c, vi); s_inter[c] = 0u; }
        }
        if (tid < L) {
            const uint32_t vh = s_hist[tid];
            if (vh) { atomicAdd(hist + (size_t)(owned - 1) * L + tid, vh); s_hist[tid] = 0u; }
        }
    };
    const int t_end = min(n_tiles, ((int)blockIdx.x + 1) * VTX_TILES_PER_WG);
    for (int t = (int)blockIdx.x * VTX_TILES_PER_WG; t < t_end; ++t) {
        __syncthreads();                                        // the tile before is done with s_keys and s_pick
        load_key_tile<KZ, 0>(s_keys, keys, tile_origin<0>(t, tiles_x, tiles_y), a.D, a.H, a.W);
        if (tid == 0) s_pick = NO_PICK;
        __syncthreads();
        // the lane's voxels: row = wave * (ROWS / 4) + it of the tile, column = lane
        int pick = NO_PICK;
#pragma unroll
        for (int it = ROWS / 4 - 1; it >= 0; --it) {
            const int row = wave * (ROWS / 4) + it;
            const int k = s_keys[(row / VTX_TY) * (KX * KY) + (row % VTX_TY + 1) * KX + 1 + lane];
            if (k) pick = (((it * 4 + wave) * 64 + lane) << 13) | (k >> 8);
        }
        if (pick != NO_PICK) atomicMin(&s_pick, pick);
        __syncthreads();
        const int lead = s_pick == NO_PICK ? 0 : (s_pick & 0x1FFF);
        if (lead == 0) continue;                                // (uniform) no voxel of any component in the tile
        if (LDS_TABLE && lead != owned) {
            if (owned) flush();
            owned = lead;
            __syncthreads();
        }
#pragma unroll 1
        for (int it = 0; it < ROWS / 4; ++it) {
            const int row = wave * (ROWS / 4) + it;
            const int *const p = s_keys + (row / VTX_TY) * (KX * KY) + (row % VTX_TY + 1) * KX + 1 + lane;
            const int k = *p;
            const int id = k >> 8, i = k & 255;                 // (id 0: no component; then nothing below counts)
            const bool in_lds = LDS_TABLE && id == owned;
            const bool in_mem = id != 0 && !in_lds;
            if (LDS_TABLE) merged_add<MERGE>(s_hist, in_lds, (unsigned)i);
            merged_add<MERGE>(hist, in_mem, (unsigned)((id - 1) * L + i));
            const unsigned mem_base = (unsigned)(id - 1) * (unsigned)LL + (unsigned)(i * L);     // (below 2^22)
            auto offset = [&](int dx, int dy, int dz, uint32_t *s_tab, uint32_t *g_tab) {
                const int kq = p[dz * (KX * KY) + dy * KX + dx];
                const bool pair = id != 0 && (kq >> 8) == id;
                const int j = kq & 255;
                if (LDS_TABLE) merged_add<MERGE>(s_tab, pair && in_lds, (unsigned)(i * L + j));
                merged_add<MERGE>(g_tab, pair && !in_lds, mem_base + (unsigned)j);
            };
            if (do_axial) {
                offset(1, 0, 0, s_axial, axial);
                offset(-1, 1, 0, s_axial, axial);
                offset(0, 1, 0, s_axial, axial);
                offset(1, 1, 0, s_axial, axial);
            }
            if (do_inter) {
#pragma unroll
                for (int dy = -1; dy <= 1; ++dy)
#pragma unroll
                    for (int dx = -1; dx <= 1; ++dx) offset(dx, dy, 1, s_inter, inter);
            }
        }
    }
    if (LDS_TABLE && owned) {
        __syncthreads();
        flush();
    }
}

// ---- finish: a workgroup per component ---------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_vtx_finish(const int2 *__restrict__ range, int L, int want, const uint32_t *__restrict__ hist,
                                                    uint32_t *inter, const uint32_t *__restrict__ axial, mi_unet_vtexture *table)
{
    __shared__ long long s_sum[4][4];
    const int r = blockIdx.x, LL = L * L;
    const bool do_axial = want & VTX_WANT_AXIAL, do_inter = want & VTX_WANT_INTER;
    long long all = 0, ax = 0, used = 0, voxels = 0;
    if (do_axial || do_inter)
        for (int c = threadIdx.x; c < LL; c += WG) {
            const uint32_t va = do_axial ? axial[(size_t)r * LL + c] : 0u;
            ax += va;
            if (do_inter) {
                const uint32_t v = inter[(size_t)r * LL + c] + va;       // (below 13 * 2^28)
                inter[(size_t)r * LL + c] = v;
                all += v;
            }
        }
    if ((int)threadIdx.x < L) {                                 // (L <= 64: the first wave)
        voxels = hist[(size_t)r * L + threadIdx.x];
        used = voxels != 0;
    }
    all = wave_sum(all); ax = wave_sum(ax); used = wave_sum(used); voxels = wave_sum(voxels);
    if ((threadIdx.x & 63) == 0) {
        s_sum[0][threadIdx.x >> 6] = all; s_sum[1][threadIdx.x >> 6] = ax; s_sum[2][threadIdx.x >> 6] = used; s_sum[3][threadIdx.x >> 6] = voxels;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        const int2 rg = range[r];
        mi_unet_vtexture t;
        t.voxels = (int32_t)s_sum[3][0];                        // (the histogram's sum; its lanes are the first wave)
        t.imin = t.voxels ? 65535 - rg.x : 0;
        t.imax = rg.y;
        t.levels_used = (int32_t)(s_sum[2][0] + s_sum[2][1] + s_sum[2][2] + s_sum[2][3]);
        t.pairs = s_sum[0][0] + s_sum[0][1] + s_sum[0][2] + s_sum[0][3];
        t.pairs_axial = s_sum[1][0] + s_sum[1][1] + s_sum[1][2] + s_sum[1][3];
        table[r] = t;
    }
}

// What the kernels' own arithmetic assumes (the entry points check the arguments and say what is wrong): an index of a voxel and of a
// cell in 32 bits, a component's number and a level in one key, an L x L table in LDS, a divisor that is not 0.
bool fits(const VolumeTextureArgs &a)
{
    if (a.D < 1 || a.H < 1 || a.W < 1 || (long long)a.D * a.H * a.W > MI_UNET_VTEX_MAX_VOXELS) return false;
    if (a.m < 1 || a.m > MI_UNET_VOLUME_MAX_TABLE || a.L < 1 || a.L > MI_UNET_VTEX_MAX_LEVELS) return false;
    return (long long)a.m * a.L * a.L <= MI_UNET_VTEX_MAX_CELLS && a.width >= 1;
}

inline unsigned blocks(unsigned n) { return (n + WG - 1) / WG; }

}  // namespace vtx

hipError_t launch_volume_texture_keys(int32_t *ids, const uint16_t *intensity, const VolumeTextureArgs &a, int2 *range, hipStream_t s)
{
    if (!ids || !intensity || !range || !vtx::fits(a)) return hipErrorInvalidValue;
    const unsigned dhw = (unsigned)a.D * (unsigned)a.H * (unsigned)a.W;
    if (hipError_t e = hipMemsetAsync(range, 0, (size_t)a.m * sizeof(int2), s)) return e;
    const unsigned waves = (dhw + 64u * vtx::RUN - 1) / (64u * vtx::RUN);
    hipLaunchKernelGGL(vtx::k_vtx_range, dim3((waves + 3) / 4), dim3(vtx::WG), 0, s, ids, intensity, dhw, a.m, range);
    if (hipError_t e = hipGetLastError()) return e;
    hipLaunchKernelGGL(vtx::k_vtx_keys, dim3(vtx::blocks(dhw)), dim3(vtx::WG), 0, s, ids, intensity, dhw, a, range);
    return hipGetLastError();
}

hipError_t launch_volume_texture_pairs(const int32_t *keys, const VolumeTextureArgs &a, int want, bool lds_table, uint32_t *hist,
                                       uint32_t *inter, uint32_t *axial, hipStream_t s)
{
    if (!keys || !hist || !inter || !axial || !vtx::fits(a) || (want & ~(VTX_WANT_AXIAL | VTX_WANT_INTER))) return hipErrorInvalidValue;
    const size_t cells = (size_t)a.m * a.L * a.L;
    if (hipError_t e = hipMemsetAsync(hist, 0, (size_t)a.m * a.L * sizeof(uint32_t), s)) return e;
    if (hipError_t e = hipMemsetAsync(inter, 0, cells * sizeof(uint32_t), s)) return e;
    if (hipError_t e = hipMemsetAsync(axial, 0, cells * sizeof(uint32_t), s)) return e;
    const int tiles_x = (a.W + VTX_TX - 1) / VTX_TX, tiles_y = (a.H + VTX_TY - 1) / VTX_TY, tiles_z = (a.D + VTX_TZ - 1) / VTX_TZ;
    const int n_tiles = tiles_x * tiles_y * tiles_z;            // (at most 2^21: a side is at most 8192 and the volume 2^28)
    const unsigned grid = (unsigned)((n_tiles + VTX_TILES_PER_WG - 1) / VTX_TILES_PER_WG);
    const size_t lds = (size_t)vtx::TILE_KEYS * sizeof(int) + (lds_table ? (size_t)(2 * a.L * a.L + a.L) * sizeof(uint32_t) : 0);
    if (lds_table)
        hipLaunchKernelGGL(vtx::k_vtx_pairs<true>, dim3(grid), dim3(vtx::WG), lds, s, keys, a, want, tiles_x, tiles_y, n_tiles, hist, inter, axial);
    else
        hipLaunchKernelGGL(vtx::k_vtx_pairs<false>, dim3(grid), dim3(vtx::WG), lds, s, keys, a, want, tiles_x, tiles_y, n_tiles, hist, inter, axial);
    return hipGetLastError();
}

hipError_t launch_volume_texture_finish(const int2 *range, const VolumeTextureArgs &a, int want, const uint32_t *hist, uint32_t *inter,
                                        const uint32_t *axial, ::mi_unet_vtexture *table, hipStream_t s)
{
    if (!range || !hist || !inter || !axial || !table || !vtx::fits(a)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(vtx::k_vtx_finish, dim3((unsigned)a.m), dim3(vtx::WG), 0, s, range, a.L, want, hist, inter, axial, table);
    return hipGetLastError();
}

}  // namespace miunet
