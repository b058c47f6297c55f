// key_tile.h -- the tile of keys with its halo in LDS that the hot paths of the texture stages walk (k_vtx_pairs, k_vzn_runs,
// k_vnb_gather): a workgroup of four waves takes a tile of TZ x TY x TX voxels, a wave per row of 64, and first
// loads the tile's keys with one voxel of halo in x and y and, in z, Z_BEFORE slices before the tile and KZ - TZ - Z_BEFORE behind it.
// A position outside the volume holds 0, the key of no component.  Internal to libmiunet.so, device code only.  gfx950 only.
#pragma once
#include "kernels.h"

namespace miunet {

namespace key_tile {

constexpr int TX = VTX_TX, TY = VTX_TY, TZ = VTX_TZ;       // 7.15's tile
constexpr int KX = TX + 2, KY = TY + 2;                     // a slice of the tile with its halo: x - 1 .. x + 1, y - 1 .. y + 1
constexpr int ROWS = TY * TZ;                               // rows of 64 voxels in a tile, ROWS / 4 per wave
constexpr int LANES = 256;                                  // of the workgroup that loads and walks a tile
static_assert(TX == 64, "a wave per row of the tile");
static_assert(ROWS % 4 == 0, "the rows of a tile are shared out among four waves");

// the volume's position of the tile's key (0, 0, 0): tiles are numbered along x first, then y, then z
template <int Z_BEFORE>
__device__ __forceinline__ int3 tile_origin(int t, int tiles_x, int tiles_y)
{
    const int tx = t % tiles_x, ty = (t / tiles_x) % tiles_y, tz = t / (tiles_x * tiles_y);
    return make_int3(tx * TX - 1, ty * TY - 1, tz * TZ - Z_BEFORE);
}

// s_keys[(lz * KY + ly) * KX + lx] = the key at o + (lx, ly, lz), KZ slices; the caller puts the barriers around it
template <int KZ, int Z_BEFORE>
__device__ __forceinline__ void load_key_tile(int *s_keys, const int32_t *__restrict__ keys, int3 o, int D, int H, int W)
{
    for (int e = threadIdx.x; e < KX * KY * KZ; e += LANES) {
        const int lz = e / (KX * KY), rem = e - lz * (KX * KY), ly = rem / KX, lx = rem - ly * KX;
        const int gx = o.x + lx, gy = o.y + ly, gz = o.z + lz;
        int k = 0;
        if (gx >= 0 && gx < W && gy >= 0 && gy < H && (Z_BEFORE == 0 || gz >= 0) && gz < D) k = keys[((size_t)gz * H + gy) * W + gx];
        s_keys[e] = k;
    }
}

// ---- the walk of a tile loaded with one voxel of halo on every side (KZ = TZ + 2, Z_BEFORE = 1) by the sweeps that need all 26 neighbours
// (k_vsk_ends, k_vsk_stats, k_vbr_classify): body(i, inside, v, code) for every row of the tile inside the volume, wave-uniformly (a wave
// per row of 64; a lane past W has inside false and v = 0): i the voxel's index, v its key, code its 26 same-key bits in raster order
// without the centre
template <class F>
__device__ __forceinline__ void walk_tile(const int *s_keys, int3 o, int D, int H, int W, F body)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int it = 0; it < ROWS / 4; ++it) {
        const int row = wave * (ROWS / 4) + it, lz = row / TY + 1, ly = row % TY + 1, lx = lane + 1;
        const int gx = o.x + lx, gy = o.y + ly, gz = o.z + lz;
        if (gy >= H || gz >= D) continue;                       // (wave-uniform)
        const int *const c = s_keys + (lz * KY + ly) * KX + lx;
        const int v = gx < W ? *c : 0;
        uint32_t code = 0;
        if (v) {
            int bit = 0;
#pragma unroll
            for (int dz = -1; dz <= 1; ++dz)
#pragma unroll
                for (int dy = -1; dy <= 1; ++dy)
#pragma unroll
                    for (int dx = -1; dx <= 1; ++dx) {
                        if (!dz && !dy && !dx) continue;
                        code |= (uint32_t)(c[(dz * KY + dy) * KX + dx] == v) << bit;
                        ++bit;
                    }
        }
        body(((size_t)gz * H + gy) * W + gx, gx < W, v, code);
    }
}

}  // namespace key_tile

}  // namespace miunet
